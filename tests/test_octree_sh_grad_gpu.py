"""K19 on the GPU: the gradient walk through SH leaves and the wide per-leaf sums
(``ops.octree_render_volume_sh_backward``), the projection (``ops.octree_project_sh``),
``OctreeSHField``, ``fit_octree_sh`` and ``scripts/train_octree.py`` on an SH file, against the
float64 restatement of the gradient contract (tests/octree_sh_grad_reference.py).  Exact f32 only:
there is no matrix work.  No reference file is read.

Every leaf's gradient is held against its budget, channel by channel (derived in the restatement).
Rays whose margin does not exceed ``ray_budget`` are left out of both sides by a zero upstream
gradient; at most 2 % of a case -- asserted here, and for the shared cases in
tests/test_octree_sh_grad_cpu.py."""

import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import octree_grad_reference as gref
from tests import octree_sh_grad_reference as sgref
from tests import octree_walk_reference as wref
from tests.octree_lattice_helpers import grid_tree, level_cells
from tests.octree_render_helpers import LEFT_OUT_CAP, camera_rays, ray_budget
from tests.octree_sh_helpers import DEGREES, SIZES, TREES, case, prefix, sh_leaf_data
from tests.octree_volume_helpers import hand_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_MINS = [0.0, float(np.float32(0.7))]
MIN_TS = [0.0, 1e-3]
BG = (0.25, 0.5, 0.125)
Y0 = 0.28209479177387814
STRIDE = {1: 16, 2: 28}


def bits(x):
    if torch.is_tensor(x):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def cuda(x, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(x, dtype)).cuda()


def upstream(count, seed, ok=None):
    rng = np.random.default_rng(seed)
    d_color = rng.normal(size=(count, 3)).astype(np.float32)
    d_alpha = rng.normal(size=count).astype(np.float32)
    if ok is not None:
        d_color[~ok] = 0
        d_alpha[~ok] = 0
    return d_color, d_alpha


def tree_depth(nodes, leaves):
    import fourier_feature_nets as ffn
    return ffn.OcTree(1.0, nodes, leaves).depth


def device_rows(scale, nodes, leaves, data, degree, starts, dirs, d_color, d_alpha, t_min=0.0,
                background=BG, min_t=0.0, workspace=None):
    """-> the (L, stride) device rows of the gradient, as a device tensor."""
    from fourier_feature_nets_amd import ops
    rows = cuda(ops.octree_sh_device_layout(data, degree))
    return ops.octree_render_volume_sh_backward(
        cuda(starts), cuda(dirs), float(scale), tree_depth(nodes, leaves), cuda(nodes, np.int64),
        cuda(leaves, np.int64), rows, degree, cuda(d_color), cuda(d_alpha), float(t_min),
        background, float(min_t), workspace)


def device_gradient(scale, nodes, leaves, data, degree, *args, **kwargs):
    """-> (L, 3B+1) numpy in the file's order; the padding is asserted +0 on the way."""
    from fourier_feature_nets_amd import ops
    rows = device_rows(scale, nodes, leaves, data, degree, *args, **kwargs)
    assert rows.shape == (len(leaves), STRIDE[degree]) and rows.dtype == torch.float32
    rows = rows.cpu().numpy()
    assert (bits(rows[:, data.shape[1]:]) == 0).all()
    return ops.octree_sh_file_layout(rows, degree)


def worst_ratio(got, g):
    err = np.abs(got.astype(np.float64) - g["grad"])
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(g["budget"] > 0, err / g["budget"], np.where(err > 0, np.inf, 0.0))


def check(what, scale, nodes, leaves, data, degree, starts, dirs, w, ok, t_min=0.0, min_t=0.0,
          seed=9):
    left_out = 1.0 - ok.mean()
    assert left_out <= LEFT_OUT_CAP
    d_color, d_alpha = upstream(len(starts), seed, ok)
    g = sgref.gradient(w, scale, starts, dirs, data, degree, d_color, d_alpha, t_min, BG, min_t)
    got = device_gradient(scale, nodes, leaves, data, degree, starts, dirs, d_color, d_alpha,
                          t_min, BG, min_t)
    ratio = worst_ratio(got, g)
    print("%s degree %d t_min=%.2f min_T=%g: %d rays, %.4f left out, %d of %d leaves taken, longest "
          "list %d; worst error / budget: coefficients %.3f sigma %.3f"
          % (what, degree, t_min, min_t, len(starts), left_out, (g["taken"] > 0).sum(), len(data),
             g["taken"].max(), ratio[:, :-1].max(), ratio[:, -1].max()))
    assert np.isfinite(got).all()
    assert (ratio <= 1.0).all()
    assert (bits(got[g["taken"] == 0]) == 0).all()
    return got, g, (d_color, d_alpha)


# --------------------------------------------------------------------------------- one leaf
@pytest.mark.parametrize("degree", DEGREES)
def test_one_leaf_one_ray_closed_form(degree):
    bases = (degree + 1) ** 2
    nodes, leaves = np.zeros(0, np.int64), np.array([0], np.int64)
    scale = np.float32(1.0)
    # hand-written coefficients: k_cb = (c + 1) / 2 - b / 4, density 0.75
    data = np.float32([[(c + 1) / 2 - b / 4 for c in range(3) for b in range(bases)] + [0.75]])
    start, d = np.float32([[-2.5, -1.25, 2.25]]), np.float32([[2, 1, -2]])      # |d| = 3
    g_c, g_a = np.float32([[0.5, -1.0, 2.0]]), np.float32([0.25])
    o64, d64 = start[0].astype(np.float64), d[0].astype(np.float64)
    near, far = (-np.sign(d64) - o64) / d64, (np.sign(d64) - o64) / d64
    length = (far.min() - near.max()) * 3.0
    assert length > 1.0
    x, y, z = d64 / 3.0
    basis = [Y0, -0.4886025119029199 * y, 0.4886025119029199 * z, -0.4886025119029199 * x,
             1.0925484305920792 * x * y, -1.0925484305920792 * y * z,
             0.31539156525252005 * (2 * z * z - x * x - y * y), -1.0925484305920792 * x * z,
             0.5462742152960396 * (x * x - y * y)][:bases]
    k = data[0, :-1].astype(np.float64).reshape(3, bases)
    c = 1.0 / (1.0 + np.exp(-(k * np.array(basis)).sum(1)))
    a = 1.0 - np.exp(-0.75 * length)
    bg = np.float64(BG)
    # one leaf: w = a, T_2 = 1 - a, S_1 = T_2 bg
    d_k = (a * g_c[0] * c * (1 - c))[:, None] * np.array(basis)[None, :]
    d_sigma = length * ((g_c[0] * ((1 - a) * c - (1 - a) * bg)).sum() + g_a[0] * (1 - a))
    want = np.concatenate([d_k.reshape(-1), [d_sigma]])
    w = wref.walk(scale, nodes, leaves, start, d)
    g = sgref.gradient(w, scale, start, d, data, degree, g_c, g_a, 0.0, BG)
    assert np.allclose(g["grad"][0], want, rtol=1e-12, atol=1e-15)
    got = device_gradient(scale, nodes, leaves, data, degree, start, d, g_c, g_a)
    err = np.abs(got[0] - want)
    print("one leaf, degree %d: worst error / budget %.3f" % (degree, (err / g["budget"][0]).max()))
    assert (g["budget"][0] > 0).all() and (err <= g["budget"][0]).all()
    assert (got[0] != 0).all()


# ----------------------------------------------------------------------- gradient within budget
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("degree", DEGREES)
@pytest.mark.parametrize("name", ["eight", "mixed4"])
def test_gradient_within_budget(name, degree, n):
    scale, nodes, leaves, starts, directions, w, ok = case(name)
    data = sh_leaf_data(scale, leaves, degree)
    for t_min in T_MINS:
        for min_t in MIN_TS:
            check(name, scale, nodes, leaves, data, degree, starts[:n], directions[:n],
                  prefix(w, n), ok[:n], t_min, min_t)


@pytest.mark.parametrize("degree", DEGREES)
def test_density_gate(degree):
    """d sigma is 0 where the stored density is negative or NaN and passes where it is exactly 0;
    the coefficients of such a leaf still get their gradient (its weight is 0, so that gradient is
    0 too, but the leaves behind it are reached)."""
    scale, nodes, leaves, starts, directions, w, ok = case("mixed4")
    data = sh_leaf_data(scale, leaves, degree)
    busiest = np.argsort(-np.bincount(w["leaf"][w["leaf"] >= 0], minlength=len(leaves)))
    negative, nan, zero = busiest[0], busiest[2], busiest[4]
    data[negative, -1], data[nan, -1], data[zero, -1] = -1.0, np.nan, 0.0
    for t_min, min_t in ((0.0, 0.0), (T_MINS[1], 1e-3)):
        got, g, _ = check("density gate", scale, nodes, leaves, data, degree, starts, directions, w,
                          ok, t_min, min_t)
        assert g["taken"][[negative, nan, zero]].min() > 50
        assert bits(got[negative, -1]) == 0 and bits(got[nan, -1]) == 0
        assert g["grad"][negative, -1] == 0 and g["grad"][nan, -1] == 0
        # exactly 0 passes: the gradient is there, and far outside its budget from 0
        assert got[zero, -1] != 0 and abs(g["grad"][zero, -1]) > 2 * g["budget"][zero, -1]
        # a leaf without density has weight 0: no gradient for its coefficients
        assert (bits(got[[negative, nan, zero], :-1]) << 1 == 0).all()


@pytest.mark.parametrize("degree", DEGREES)
def test_wrong_restatements_miss_the_budget(degree):
    """The comparison of test_gradient_within_budget can fail: against the basis of -u, against c
    in place of c (1 - c), and against the longest list without its last entry, it does."""
    name = "mixed4"
    scale, nodes, leaves, starts, directions, w, ok = case(name)
    data = sh_leaf_data(scale, leaves, degree)
    got, g, (d_color, d_alpha) = check(name, scale, nodes, leaves, data, degree, starts, directions,
                                       w, ok)
    closest = {}
    for variant in ("flipped", "slope", "short"):
        wrong = sgref.gradient(w, scale, starts, directions, data, degree, d_color, d_alpha, 0.0, BG,
                               variant=variant)
        ratio = worst_ratio(got, dict(grad=wrong["grad"], budget=g["budget"]))
        closest[variant] = ratio.max()
        assert ratio.max() > 1.0, variant
        if variant == "short":
            assert ratio[wrong["dropped"]].max() > 1.0
    print("degree %d, wrong restatements, worst error / budget: %s (the right one: %.3f)"
          % (degree, ", ".join("%s %.3g" % item for item in closest.items()),
             worst_ratio(got, g).max()))


# --------------------------------------------------------------------------- band-0 reduction
@pytest.mark.parametrize("degree", DEGREES)
def test_band_zero_reduction_to_k17(degree):
    from fourier_feature_nets_amd import ops
    bases = (degree + 1) ** 2
    scale, nodes, leaves, starts, directions, w, ok = case("mixed4")
    data = sh_leaf_data(scale, leaves, degree)
    for c in range(3):
        data[:, c * bases + 1:(c + 1) * bases] = 0.0
    logits = np.zeros((len(data), 4), np.float32)
    for c in range(3):
        logits[:, c] = data[:, c * bases] * np.float32(Y0)        # the kernel's first product
    plain = ops.octree_bake(cuda(logits)).cpu().numpy()
    plain[:, 3] = data[:, -1]
    d_color, d_alpha = upstream(len(starts), 21, ok)
    depth = tree_depth(nodes, leaves)
    for t_min, min_t in ((0.0, 0.0), (T_MINS[1], 1e-3)):
        got = device_gradient(scale, nodes, leaves, data, degree, starts, directions, d_color,
                              d_alpha, t_min, BG, min_t)
        k17 = ops.octree_render_volume_backward(
            cuda(starts), cuda(directions), float(scale), depth, cuda(nodes, np.int64),
            cuda(leaves, np.int64), cuda(plain), cuda(d_color), cuda(d_alpha), t_min, BG,
            min_t).cpu().numpy()
        assert np.array_equal(bits(got[:, -1]), bits(k17[:, 3]))
        assert (got[:, -1] != 0).any()
        g = sgref.gradient(w, scale, starts, directions, data, degree, d_color, d_alpha, t_min, BG,
                           min_t)
        k = gref.gradient(w, scale, starts, directions, plain, d_color, d_alpha, t_min, BG, min_t)
        for c in range(3):
            p = plain[:, c].astype(np.float64)
            want = Y0 * p * (1.0 - p) * k["grad"][:, c]
            assert (np.abs(got[:, c * bases] - want) <= g["budget"][:, c * bases]).all()
        assert (worst_ratio(got, g) <= 1.0).all()


# ----------------------------------------------------------------------------- the field
def sh_tree(scale, nodes, leaves, data, degree):
    import fourier_feature_nets as ffn
    tree = ffn.OcTree(float(scale), nodes, leaves, data, sh_degree=degree)
    tree._center = (0.0, 0.0, 0.0)
    return tree


@pytest.mark.parametrize("degree", DEGREES)
def test_forward_identity(degree):
    import fourier_feature_nets as ffn
    scale, nodes, leaves, starts, directions, _, _ = case("mixed4")
    data = sh_leaf_data(scale, leaves, degree)
    tree = sh_tree(scale, nodes, leaves, data, degree)
    field = ffn.OctreeSHField(tree)
    assert field.data.shape == (len(data), STRIDE[degree]) and field.data.is_cuda
    assert field.data.requires_grad and field.sh_degree == degree
    dev_s, dev_d = cuda(starts), cuda(directions)
    for t_min, min_t in ((0.0, 0.0), (T_MINS[1], 1e-3)):
        want = tree.render_volume(dev_s, dev_d, t_min, BG, min_t)
        out = field(dev_s, dev_d, t_min, BG, min_t)
        assert type(out).__name__ == "RenderResult"
        for a, b in zip(out, want):
            assert torch.is_tensor(a) and a.is_cuda and np.array_equal(bits(a), bits(b))
    out = field(dev_s, dev_d, 0.0, BG)
    d_color, d_alpha = upstream(len(starts), 4)
    (out.color * cuda(d_color)).sum().add((out.alpha * cuda(d_alpha)).sum()).backward()
    direct = device_rows(scale, nodes, leaves, data, degree, starts, directions, d_color, d_alpha)
    assert np.array_equal(bits(field.data.grad), bits(direct))
    assert (bits(field.data.grad[:, data.shape[1]:]) == 0).all()
    again = field.tree()
    assert again is not tree and again.center == tree.center and again.sh_degree == degree
    assert np.array_equal(again.state_dict["leaf_index"], tree.state_dict["leaf_index"])
    assert np.array_equal(again.state_dict["node_index"], tree.state_dict["node_index"])
    assert np.array_equal(bits(again.leaf_data()), bits(data))


# ------------------------------------------------------------------- the wide reduce's edges
@functools.lru_cache(maxsize=None)
def complete_tree():
    """The complete depth-2 tree: eight leaves, slot 4 [x upper] + 2 [y upper] + [z upper]; a +x
    ray takes the lower and the upper leaf of its y-z quadrant."""
    nodes, leaves = grid_tree(2, level_cells(1))
    return np.float32(1.0), nodes, leaves


def axis_rays(rng, count, lo=-1.0, hi=1.0, x=-2.0):
    """+x rays from x = ``x`` at random y, z in (lo, hi): off every plane with probability 1."""
    starts = np.empty((count, 3), np.float32)
    starts[:, 0] = x
    starts[:, 1:] = rng.uniform(lo, hi, (count, 2))
    return starts, np.tile(np.float32([1, 0, 0]), (count, 1))


def quadrant_rays(rng, through, inside):
    """Per y-z quadrant q (y upper: 2, z upper: 1): ``through[q]`` rays from x = -2 (two leaves,
    slots q and 4 + q) and ``inside[q]`` rays from x = 0.5 (the upper leaf only), shuffled."""
    starts, dirs = [], []
    for q in range(4):
        y, z = (0.0, 1.0) if q & 2 else (-1.0, 0.0), (0.0, 1.0) if q & 1 else (-1.0, 0.0)
        for count, x in ((through[q], -2.0), (inside[q], 0.5)):
            s, d = axis_rays(rng, count, 0.0, 1.0, x)
            s[:, 1] = y[0] + s[:, 1] * (y[1] - y[0])
            s[:, 2] = z[0] + s[:, 2] * (z[1] - z[0])
            starts.append(s)
            dirs.append(d)
    starts, dirs = np.concatenate(starts), np.concatenate(dirs)
    order = rng.permutation(len(starts))
    return starts[order], dirs[order]


def check_lists(what, degree, through, inside, seed):
    scale, nodes, leaves = complete_tree()
    data = sh_leaf_data(scale, leaves, degree)
    starts, dirs = quadrant_rays(np.random.default_rng(seed), through, inside)
    w = wref.walk(scale, nodes, leaves, starts, dirs)
    ok = ~w["hit"] | (w["margin"] > ray_budget(w, scale, starts, dirs))
    assert ok.all()
    got, g, up = check(what, scale, nodes, leaves, data, degree, starts, dirs, w, ok)
    lengths = [through[q] for q in range(4)] + [through[q] + inside[q] for q in range(4)]
    assert g["taken"].tolist() == lengths
    return got, g, up, (scale, nodes, leaves, data, starts, dirs, w)


@pytest.mark.parametrize("degree", DEGREES)
@pytest.mark.parametrize("launch", [0, 1, 2])
def test_list_lengths_at_the_reduce_chunk(launch, degree):
    """The list lengths share launches: the lists are those of the eight leaves of the complete
    depth-2 tree (a +x ray takes the lower and the upper leaf of its quadrant), several lengths per
    launch, each one a leaf's whole list and asserted through the restatement's ``taken``.  Launch
    0: 1, 15, 16, 17, 255, 256, 257 (and 4095); launch 1: 4096 and 4097; launch 2: 1, 17, 16, 0, 33
    in leaf order, for the compact placement of the partial rows."""
    through, inside = [([1, 15, 16, 255], [16, 241, 241, 3840]), ([4096, 0, 0, 0], [1, 0, 0, 0]),
                       ([1, 17, 16, 0], [32, 0, 0, 0])][launch]
    got, g, up, (scale, nodes, leaves, data, starts, dirs, w) = check_lists(
        "list lengths, launch %d" % launch, degree, through, inside, 70 + launch)
    want = [{1, 15, 16, 17, 255, 256, 257}, {4096, 4097}, {0, 1, 16, 17, 33}][launch]
    assert want <= set(g["taken"].tolist())
    if launch == 2:
        assert g["taken"].tolist()[:5] == [1, 17, 16, 0, 33]      # compact placement, in order
    if launch == 1:
        wrong = sgref.gradient(w, scale, starts, dirs, data, degree, up[0], up[1], 0.0, BG,
                               variant="short")
        assert wrong["dropped"] == 4 and g["taken"][4] == 4097
        assert not (np.abs(got[4] - wrong["grad"][4]) <= g["budget"][4]).all()


@pytest.mark.parametrize("degree", DEGREES)
@pytest.mark.parametrize("entries", [1, 1024, 1025])
def test_entry_counts_at_the_sort_tile(entries, degree):
    two = entries // 2
    through = [two // 4 + (q < two % 4) for q in range(4)]
    _, g, _, _ = check_lists("E = %d" % entries, degree, through, [entries - 2 * two, 0, 0, 0],
                             entries)
    assert g["taken"].sum() == entries


@pytest.mark.parametrize("degree", DEGREES)
@pytest.mark.parametrize("count", [1, 2, 257])
def test_leaf_counts_at_the_sort_passes(count, degree):
    """L = 1: no sort pass (the entries stay in place); 2: one; 257: two."""
    rng = np.random.default_rng(count)
    if count == 1:
        scale, nodes, leaves = np.float32(2.0), np.zeros(0, np.int64), np.array([0], np.int64)
        starts, dirs = camera_rays(rng, 3000, scale)
    else:
        # level-3 cells of a depth-4 tree, a seeded draw that always holds the two ends of the row
        # of cells at the top of y and z (the second of them is the largest id, the last leaf)
        top = 7
        cells = {(3, 0, top, top), (3, top, top, top)}
        for cell in rng.permutation(level_cells(3, rng, count)).tolist():
            if len(cells) == count:
                break
            cells.add(tuple(cell))
        nodes, leaves = grid_tree(4, sorted(cells))
        scale = np.float32(1.0)
        rng = np.random.default_rng(count + 1)
        cam_s, cam_d = camera_rays(rng, 3000, scale)
        # into the last cell along the row at the top of y and z, from inside the cell before it
        ax_s, ax_d = axis_rays(rng, 64, 0.75, 1.0, 1.0 - 1.5 * 0.25)
        starts, dirs = np.concatenate([cam_s, ax_s]), np.concatenate([cam_d, ax_d])
    assert len(leaves) == count
    data = sh_leaf_data(scale, leaves, degree)
    w = wref.walk(scale, nodes, leaves, starts, dirs)
    ok = ~w["hit"] | (w["margin"] > ray_budget(w, scale, starts, dirs))
    _, g, _ = check("L = %d" % count, scale, nodes, leaves, data, degree, starts, dirs, w, ok)
    taken = np.nonzero(g["taken"])[0]
    assert len(taken) >= min(count, 2)
    if count == 257:
        assert (taken >> 8).max() == 1                  # the second key byte differs


# ------------------------------------------------------------------------------ workspace
@pytest.mark.parametrize("degree", DEGREES)
def test_exact_workspace_refusal_and_growth(degree):
    from fourier_feature_nets_amd import _lib, ops
    scale, nodes, leaves = complete_tree()
    data = sh_leaf_data(scale, leaves, degree)
    count = 2000
    starts, dirs = axis_rays(np.random.default_rng(3), count)
    d_color, d_alpha = upstream(count, 3)
    first = ops.OctreeGradSHWorkspace(degree)
    plain = device_rows(scale, nodes, leaves, data, degree, starts, dirs, d_color, d_alpha,
                        workspace=first)
    entries = first.entries
    assert entries == 2 * count

    def sized(max_entries):
        ws = ops.OctreeGradSHWorkspace(degree)
        need = ops.octree_grad_sh_workspace_bytes(count, len(leaves), max_entries, degree)
        assert need % 4 == 0
        ws.buffer = torch.empty((need // 4,), dtype=torch.float32, device="cuda")
        ws.max_entries, ws.shape = max_entries, (count, len(leaves))
        return ws

    exact = device_rows(scale, nodes, leaves, data, degree, starts, dirs, d_color, d_alpha,
                        workspace=sized(entries))
    assert np.array_equal(bits(exact), bits(plain))
    # one entry short: refused with the counts in the message.  The call is made directly, since
    # the ops wrapper would grow the workspace and repeat it.
    ws = sized(entries - 1)
    out = torch.full((len(leaves), STRIDE[degree]), 7.0, device="cuda")
    told = _lib.c_i64(-1)
    dev = [cuda(starts), cuda(dirs), cuda(nodes, np.int64), cuda(leaves, np.int64),
           cuda(ops.octree_sh_device_layout(data, degree)), cuda(d_color), cuda(d_alpha)]
    with pytest.raises(_lib.FfnError, match="take %d leaves, the workspace holds %d entries"
                       % (entries, entries - 1)):
        ops._call("ffn_octree_render_volume_sh_backward",
                  *ops._walk_args(dev[0], dev[1], float(scale), 2, dev[2], dev[3]),
                  _lib.c_f(0.0), ops._dev(dev[4]), _lib.c_f(BG[0]), _lib.c_f(BG[1]),
                  _lib.c_f(BG[2]), _lib.c_f(0.0), ops._dev(dev[5]), ops._dev(dev[6]),
                  ops._dev(ws.buffer), _lib.c_i64(ws.buffer.numel() * 4),
                  _lib.c_i64(ws.max_entries), ops._dev(out), ctypes.byref(told), _lib.c_i(degree),
                  _lib.c_i(STRIDE[degree]))
    assert told.value == entries
    assert (out.cpu().numpy() == 7.0).all()                   # nothing was written
    # a first guess of one entry per ray: 2000 rays take 4000 leaves, the wrapper grows and repeats
    small = ops.OctreeGradSHWorkspace(degree, entries_per_ray=1)
    grown = device_rows(scale, nodes, leaves, data, degree, starts, dirs, d_color, d_alpha,
                        workspace=small)
    assert small.max_entries >= entries > count and small.entries == entries
    assert np.array_equal(bits(grown), bits(plain))
    # a workspace of the other degree is not taken
    with pytest.raises(ValueError, match="degree"):
        device_rows(scale, nodes, leaves, data, degree, starts, dirs, d_color, d_alpha,
                    workspace=ops.OctreeGradSHWorkspace(3 - degree))
    # below 96 bytes per additional entry (derived in the issue: K17b's 52 + 4 + 14, rounded up)
    a = ops.octree_grad_sh_workspace_bytes(4096, 100000, 1 << 17, degree)
    b = ops.octree_grad_sh_workspace_bytes(4096, 100000, (1 << 17) + (1 << 20), degree)
    assert (b - a) / float(1 << 20) < 96.0


def test_determinism():
    scale, nodes, leaves, starts, directions, _, _ = case("mixed4")
    data = sh_leaf_data(scale, leaves, 2)
    d_color, d_alpha = upstream(len(starts), 6)
    args = (scale, nodes, leaves, data, 2, starts, directions, d_color, d_alpha, 0.0, BG, 1e-3)
    first = device_rows(*args)
    second = device_rows(*args)
    assert np.array_equal(bits(first), bits(second))
    # on a side stream, while the default stream renders
    tree = sh_tree(scale, nodes, leaves, data, 2)
    side = torch.cuda.Stream()
    dev_s, dev_d = cuda(np.tile(starts, (50, 1))), cuda(np.tile(directions, (50, 1)))
    torch.cuda.synchronize()
    for _ in range(4):
        tree.render_volume(dev_s, dev_d, 0.0, BG)
    with torch.cuda.stream(side):
        third = device_rows(*args)
    torch.cuda.synchronize()
    assert np.array_equal(bits(first), bits(third))


# ------------------------------------------------------------------------- K19c and one step
@pytest.mark.parametrize("degree", DEGREES)
def test_projection_on_a_wild_row(degree):
    from fourier_feature_nets_amd import ops
    channels, stride = 3 * (degree + 1) ** 2 + 1, STRIDE[degree]
    nan = np.float32(np.nan)
    rows = np.zeros((4, stride), np.float32)
    rows[0, :channels] = np.linspace(-1e30, 1e30, channels)     # negative density, large logits
    rows[1, :channels] = nan
    rows[2, 0], rows[2, 1], rows[2, 2], rows[2, 3] = -0.0, -0.0, np.inf, -np.inf
    rows[3, 0], rows[3, 5], rows[3, channels - 1] = 2.5, nan, -7.0
    rows[:, channels:] = [[3.0, nan, -1.0][:stride - channels]] * 4      # padding: untouched
    want = rows.copy()
    want[0, 0] = 0.0
    want[1, :channels] = 0.0
    want[2, 0] = 0.0                                                # +0: the sign bit goes
    want[3, 5] = 0.0
    dev = cuda(rows)
    assert ops.octree_project_sh(dev, degree) is dev
    assert np.array_equal(bits(dev), bits(want))
    assert bits(dev)[2, 1] == 0x80000000                            # a coefficient's -0 stays
    for bad in (dev[:, :channels - 1], dev[0]):
        with pytest.raises(ValueError, match="leaf_rows"):
            ops.octree_project_sh(bad.contiguous(), degree)


@pytest.mark.parametrize("degree", DEGREES)
def test_one_step(degree):
    """K7 then K19c on the GPU gradient, against torch.optim.Adam in float64 on the restatement's
    gradient (clipped as K7 clips), then the projection.  Budget, as test_one_step of K17 derives
    it: at t = 1 the step is lr * g / (|g| + eps), whose slope in g is at most 1 / (|g| + eps), so
    the gradient's own budget scaled by the clip coefficient moves it by at most lr * b / (|g| +
    eps); the clip coefficient moves by at most the relative change of the norm; plus 8 f32
    roundings of the gradient and of the parameter."""
    from fourier_feature_nets_amd import ops
    scale, nodes, leaves, starts, directions, w, ok = case("mixed4")
    data = sh_leaf_data(scale, leaves, degree)
    d_color, d_alpha = upstream(len(starts), 13, ok)
    d_color *= np.float32(1e-3)
    d_alpha *= np.float32(1e-3)
    g = sgref.gradient(w, scale, starts, directions, data, degree, d_color, d_alpha, 0.0, BG)
    grads = device_rows(scale, nodes, leaves, data, degree, starts, directions, d_color, d_alpha)
    lr, clip, max_norm, eps = 1e-2, 0.1, 0.1, 1e-8
    params = cuda(ops.octree_sh_device_layout(data, degree))
    flat = params.view(-1)
    ops.clip_adam(flat, grads.view(-1), torch.zeros_like(flat), torch.zeros_like(flat), 1, lr,
                  clip_value=clip, max_norm=max_norm)
    ops.octree_project_sh(params, degree)
    rows = params.cpu().numpy()
    assert (bits(rows[:, data.shape[1]:]) == 0).all()           # the padding stays zero
    got = ops.octree_sh_file_layout(rows, degree).astype(np.float64)
    want = torch.tensor(data.astype(np.float64), requires_grad=True)
    clipped = np.clip(g["grad"], -clip, clip)
    norm = np.sqrt((clipped ** 2).sum())
    coef = min(1.0, max_norm / (norm + 1e-6))
    want.grad = torch.tensor(clipped * coef)
    torch.optim.Adam([want], lr=lr, eps=eps).step()
    want = want.detach().numpy()
    want[:, -1] = np.maximum(want[:, -1], 0.0)
    moved = np.abs(clipped * coef)
    coef_rel = np.sqrt((g["budget"] ** 2).sum()) / max(norm, 1e-30) + 1e-6
    budget = lr * (coef * g["budget"] + moved * coef_rel + 8 * 2.0 ** -24 * moved) / (moved + eps) \
        + 8 * 2.0 ** -24 * np.maximum(np.abs(data), lr)
    err = np.abs(got - want)
    print("one step, degree %d: clip coefficient %.3g, worst error / budget %.3f"
          % (degree, coef, (err / budget).max()))
    assert (err <= budget).all()
    assert (got[:, -1] >= 0).all() and not np.array_equal(got, data.astype(np.float64))


# --------------------------------------------------------------------------------- fitting
class _Sampler:
    """What ``fit_octree_sh`` reads of a ``RaySampler``: one 'camera' holding every ray."""

    def __init__(self, starts, directions):
        self.starts, self.directions = starts, directions
        self.num_cameras, self.rays_per_camera = 1, starts.shape[0]


class _Dataset:
    def __init__(self, sampler, colors, alphas, alpha_weight=0.1):
        self.sampler, self.colors, self.alphas = sampler, colors, alphas
        self.alpha_weight = alpha_weight

    def _gt_alphas(self):
        return self.alphas


def test_fit_loop():
    import fourier_feature_nets as ffn
    degree = 2
    scale, nodes, leaves = TREES["mixed4"]()
    data = sh_leaf_data(scale, leaves, degree)
    teacher = sh_tree(scale, nodes, leaves, data, degree)
    starts, directions = camera_rays(np.random.default_rng(31), 20000, scale)
    dev_s, dev_d = cuda(starts), cuda(directions)
    target = teacher.render_volume(dev_s, dev_d, 0.0, (0, 0, 0))
    dataset = _Dataset(_Sampler(dev_s, dev_d), target.color.contiguous(), target.alpha.contiguous())
    noise = np.random.default_rng(14).normal(size=data.shape).astype(np.float32)
    start = data.copy()
    start[:, :-1] = data[:, :-1] + 0.5 * noise[:, :-1]
    start[:, -1] = np.maximum(data[:, -1] * (1 + 0.5 * noise[:, -1]), 0)
    begin = sh_tree(scale, nodes, leaves, start.copy(), degree)
    steps = 300
    runs = []
    for _ in range(2):
        fitted, log = ffn.fit_octree_sh(begin, dataset, dataset, 4096, num_steps=steps,
                                        report_interval=150, verbose=False)
        runs.append((fitted, log))
    fitted, log = runs[0]
    assert len(log) == steps and [e.step for e in log] == list(range(steps))
    assert fitted.sh_degree == degree and fitted.center == begin.center
    assert np.array_equal(fitted.state_dict["leaf_index"], leaves)
    assert np.array_equal(fitted.state_dict["node_index"], nodes)
    assert np.array_equal(bits(begin.leaf_data()), bits(start))          # the input is unchanged
    losses = np.array([e.loss for e in log])
    assert np.isfinite(losses).all()
    first, middle, last = losses[:16].mean(), losses[steps // 2:steps // 2 + 16].mean(), \
        losses[-16:].mean()
    reports = [e for e in log if not np.isnan(e.val_psnr)]
    print("SH fit loop: loss %.6g at step 0, %.6g at the midpoint, %.6g at the end; val psnr %.2f "
          "-> %.2f" % (first, middle, last, reports[0].val_psnr, reports[-1].val_psnr))
    assert last < middle < first
    assert [e.step for e in reports] == list(range(10)) + [150]
    out = fitted.leaf_data()
    assert out.shape == data.shape and out.dtype == np.float32 and np.isfinite(out).all()
    assert (out[:, -1] >= 0).all() and not np.array_equal(out, start)
    # the second seeded run: the same log and the same tree, bit for bit
    again, log2 = runs[1]
    assert np.array_equal(bits([e.loss for e in log2]), bits(losses))
    assert np.array_equal(bits([e.val_psnr for e in log2]), bits([e.val_psnr for e in log]))
    assert np.array_equal(bits(again.leaf_data()), bits(out))


def test_train_octree_program_on_an_sh_file(tmp_path):
    import fourier_feature_nets as ffn
    data_path, tree_path, out_path = [str(tmp_path / name) for name in
                                      ("data.npz", "tree.npz", "out.npz")]
    res = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "make_synthetic_npz.py"),
                          data_path, "--size", "8", "--cameras", "4"], capture_output=True,
                         text=True, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    scale, nodes, leaves, _, _, _ = hand_case()
    data = sh_leaf_data(scale, leaves, 2)
    ffn.OcTree(float(scale), nodes, leaves, data, sh_degree=2).save(tree_path)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train_octree.py"),
                          tree_path, data_path, out_path, "--center", "0", "0", "0", "--steps",
                          "20", "--batch-size", "64", "--min-transmittance", "1e-3"],
                         capture_output=True, text=True, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    assert "SH leaves of degree 2" in res.stdout and "3 leaves fitted" in res.stdout
    fitted = ffn.OcTree.load(out_path)
    assert fitted.sh_degree == 2
    assert np.array_equal(fitted.state_dict["node_index"], nodes)
    assert np.array_equal(fitted.state_dict["leaf_index"], leaves)
    out = fitted.leaf_data()
    assert out.shape == (3, 28) and out.dtype == np.float32 and not np.array_equal(out, data)
