"""K17b (``ops.octree_render_volume_backward``: scan, radix sort, per-leaf reduce) at the edges of
its shapes, against the float64 restatement of the gradient (tests/octree_grad_reference.py) with
that restatement's own budgets.  No reference file is read.

The edges: the number of sort passes (``ceil(bits(L - 1) / 8)``: L = 2, 255, 256, 257, 65535,
65536, 65537), the number of entries E against the sort tile of 1024, the length of one leaf's
list against the reduce chunk of 16 (16 / 17, 256 / 257, 4096 / 4097), the ray count against the
scan block of 4096, and the scan's carry loop (more than 1024 blocks).

Rays are ordinary ones.  AXIS rays run along +x at random y, z off every plane, so that each takes
a known number of leaves; none of them is left out.  Camera rays keep the rule of the other
gradient tests: a ray whose margin does not exceed ``ray_budget`` gets a zero upstream gradient on
both sides, at most 2 % of a case."""

import functools

import numpy as np
import pytest
import torch

from tests import octree_grad_reference as gref
from tests import octree_walk_reference as wref
from tests.octree_lattice_helpers import grid_tree, level_cells
from tests.octree_render_helpers import LEFT_OUT_CAP, camera_rays, ray_budget
from tests.octree_volume_helpers import random_leaf_data

pytestmark = pytest.mark.gpu

BG = (0.25, 0.5, 0.125)


def bits(x):
    if torch.is_tensor(x):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def cuda(x, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(x, dtype)).cuda()


def upstream(count, seed):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(count, 3)).astype(np.float32),
            rng.normal(size=count).astype(np.float32))


def device_gradient(tree, starts, dirs, d_color, d_alpha, workspace=None):
    from fourier_feature_nets_amd import ops
    scale, depth, nodes, leaves, data = tree
    if workspace is None:
        workspace = ops.OctreeGradWorkspace()
    got = ops.octree_render_volume_backward(
        cuda(starts), cuda(dirs), float(scale), depth, cuda(nodes, np.int64),
        cuda(leaves, np.int64), cuda(data), cuda(d_color), cuda(d_alpha), 0.0, BG, 0.0, workspace)
    return got.cpu().numpy(), workspace


def check(what, tree, starts, dirs, seed=5, none_left_out=False, rows=None):
    """Device against restatement.  ``rows``: the rays the restatement walks (the others are known
    to miss the cube).  -> got, g (the restatement), w, upstream gradients, the workspace."""
    scale, depth, nodes, leaves, data = tree
    if rows is None:
        rows = np.arange(len(starts))
    w = wref.walk(scale, nodes, leaves, starts[rows], dirs[rows])
    ok = ~w["hit"] | (w["margin"] > ray_budget(w, scale, starts[rows], dirs[rows]))
    left_out = 1.0 - ok.mean()
    assert left_out <= LEFT_OUT_CAP and (left_out == 0 or not none_left_out)
    d_color, d_alpha = upstream(len(starts), seed)
    d_color[rows[~ok]] = 0
    d_alpha[rows[~ok]] = 0
    g = gref.gradient(w, scale, starts[rows], dirs[rows], data, d_color[rows], d_alpha[rows], 0.0, BG)
    got, workspace = device_gradient(tree, starts, dirs, d_color, d_alpha)
    assert got.shape == (len(leaves), 4) and np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - g["grad"])
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(g["budget"] > 0, err / g["budget"], np.where(err > 0, np.inf, 0.0))
    print("%s: %d rays, %d leaves (%d taken), E = %d, longest list %d, %.4f left out; worst error "
          "/ budget: colour %.3f sigma %.3f" %
          (what, len(starts), len(leaves), (g["taken"] > 0).sum(), g["taken"].sum(),
           g["taken"].max(), left_out, ratio[:, :3].max(), ratio[:, 3].max()))
    assert (err <= g["budget"]).all()
    assert (bits(got[g["taken"] == 0]) == 0).all()
    assert workspace.entries == g["taken"].sum()
    return got, g, w, (d_color, d_alpha), workspace


def without_last_entry(tree, starts, dirs, w, up, leaf):
    """The restatement with the last entry of ``leaf`` (that of its last ray) removed: a wrong
    reference.  The ray's upstream gradient is zeroed, which removes its entries in other leaves
    too: callers look at the row of ``leaf`` alone."""
    scale, depth, nodes, leaves, data = tree
    rays = w["ray"][(w["leaf"] == leaf) & (w["t_out"] > 0.0)]
    d_color, d_alpha = up[0].copy(), up[1].copy()
    d_color[rays.max()] = 0
    d_alpha[rays.max()] = 0
    return gref.gradient(w, scale, starts, dirs, data, d_color, d_alpha, 0.0, BG)


# ------------------------------------------------------------------------------- pass counts
@functools.lru_cache(maxsize=None)
def subset_tree(count):
    """``count`` leaves: level-3 cells of a depth-4 tree, or level-6 cells of a depth-7 tree, a
    seeded draw that always holds the two ends of the row of cells at the top of y and z (the
    second of them is the largest id, leaf ``count - 1``)."""
    rng = np.random.default_rng(count)
    level = 3 if count <= 512 else 6
    top = (1 << level) - 1
    cells = {(level, 0, top, top), (level, top, top, top)}
    for cell in rng.permutation(level_cells(level, rng, count)).tolist():
        if len(cells) == count:
            break
        cells.add(tuple(cell))
    nodes, leaves = grid_tree(level + 1, sorted(cells))
    data = random_leaf_data(np.float32(1.0), leaves)
    return np.float32(1.0), level + 1, nodes, leaves, data


def axis_rays(rng, count, lo=-1.0, hi=1.0, x=-2.0):
    """+x rays from x = ``x`` at random y, z in (lo, hi): off every plane with probability 1."""
    starts = np.empty((count, 3), np.float32)
    starts[:, 0] = x
    starts[:, 1:] = rng.uniform(lo, hi, (count, 2))
    return starts, np.tile(np.float32([1, 0, 0]), (count, 1))


@pytest.mark.parametrize("count", [2, 255, 256, 257, 65535, 65536, 65537])
def test_sort_pass_counts(count):
    tree = subset_tree(count)
    scale, depth, nodes, leaves, data = tree
    assert len(leaves) == count
    rng = np.random.default_rng(count + 1)
    # at most 4096 rays on the big trees.  About 2.5 % of camera rays graze one of the many small
    # regions of a depth-7 tree, so the axis rays (none left out) make up most of that case
    cam_s, cam_d = camera_rays(rng, 1536 if count > 512 else 3000, scale)
    all_s, all_d = axis_rays(rng, 2496 if count > 512 else 0)
    # into the last cell (the largest id) along the row at the top of y and z, from inside the
    # cell before it: the last leaf is the first or second a ray takes, so each of its entries
    # is large against its own budget (nothing in front of it to drift)
    side = 2.0 / (1 << (depth - 1))
    ax_s, ax_d = axis_rays(rng, 64, 1.0 - side, 1.0, 1.0 - 1.5 * side)
    starts, dirs = np.concatenate([cam_s, all_s, ax_s]), np.concatenate([cam_d, all_d, ax_d])
    got, g, w, up, _ = check("L = %d" % count, tree, starts, dirs)
    taken = np.nonzero(g["taken"])[0]
    assert g["taken"][count - 1] >= 32                         # the last leaf, by the axis rays
    for shift in range(0, 8 * (((count - 1).bit_length() + 7) // 8), 8):
        assert len(np.unique((taken >> shift) & 255)) >= 2      # every key byte differs
    if count == 65537:
        assert (taken >> 16).max() == 1
        leaf = count - 1
        wrong = without_last_entry(tree, starts, dirs, w, up, leaf)
        assert not (np.abs(got[leaf] - wrong["grad"][leaf]) <= wrong["budget"][leaf]).all()


# ------------------------------------------------------------- entry counts and list lengths
@functools.lru_cache(maxsize=None)
def complete_tree():
    """The complete depth-2 tree: eight leaves, slot 4 [x upper] + 2 [y upper] + [z upper]; a +x
    ray takes the lower and the upper leaf of its y-z quadrant."""
    nodes, leaves = grid_tree(2, level_cells(1))
    data = random_leaf_data(np.float32(1.0), leaves)
    return np.float32(1.0), 2, nodes, leaves, data


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


@pytest.mark.parametrize("entries", [1, 1023, 1024, 1025, 2049])
def test_entry_counts_at_the_sort_tile(entries):
    rng = np.random.default_rng(entries)
    two = entries // 2
    through = [two // 4 + (q < two % 4) for q in range(4)]
    starts, dirs = quadrant_rays(rng, through, [entries - 2 * two, 0, 0, 0])
    _, g, _, _, _ = check("E = %d" % entries, complete_tree(), starts, dirs, none_left_out=True)
    assert g["taken"].sum() == entries


@pytest.mark.parametrize("launch", [0, 1])
def test_list_lengths_at_the_reduce_chunk(launch):
    rng = np.random.default_rng(70 + launch)
    through, inside = [([1, 15, 16, 255], [16, 241, 241, 3840]), ([4096, 0, 0, 0], [1, 0, 0, 0])][launch]
    lengths = [through[q] for q in range(4)] + [through[q] + inside[q] for q in range(4)]
    want = [{1, 15, 16, 17, 255, 256, 257, 4095}, {4096, 4097}][launch]
    assert want <= set(lengths)
    tree = complete_tree()
    starts, dirs = quadrant_rays(rng, through, inside)
    got, g, w, up, _ = check("list lengths, launch %d" % launch, tree, starts, dirs,
                             none_left_out=True)
    assert g["taken"].tolist() == lengths
    if launch == 1:
        wrong = without_last_entry(tree, starts, dirs, w, up, 4)
        assert not (np.abs(got[4] - wrong["grad"][4]) <= wrong["budget"][4]).all()


# ------------------------------------------------------------------------------ ray counts
@pytest.mark.parametrize("count", [4095, 4096, 4097, 8193])
def test_ray_counts_at_the_scan_block(count):
    rng = np.random.default_rng(count)
    starts, dirs = axis_rays(rng, count)
    _, g, w, _, _ = check("n = %d" % count, complete_tree(), starts, dirs, none_left_out=True)
    assert w["hit"].all() and g["taken"].sum() == 2 * count


def test_scan_carry_loop():
    """n = 4096 * 1024 + 65: 1025 scan blocks, the smallest count at which the top kernel of the
    scan (one workgroup of 1024 threads) carries.  All rays but 1665 start outside and point away;
    the hits lie in the first block, across the block 1022 / 1023 and 1023 / 1024 boundaries and
    in the last, partial block.  depth 2: n (3 * 2 + 1) < 2^31."""
    count = 4096 * 1024 + 65
    rng = np.random.default_rng(77)
    starts = np.empty((count, 3), np.float32)
    starts[:] = np.float32([3, 3, 3])
    dirs = np.tile(np.float32([1, 0, 0]), (count, 1))
    rows = np.concatenate([np.arange(700), np.arange(4096 * 1023 - 300, 4096 * 1023 + 300),
                           np.arange(4096 * 1024 - 300, count)])
    starts[rows], _ = axis_rays(rng, len(rows))
    _, g, w, _, _ = check("carry loop", complete_tree(), starts, dirs, none_left_out=True,
                          rows=rows)
    assert w["hit"].all() and g["taken"].sum() == 2 * len(rows)


# ------------------------------------------------------------------------------ identities
def test_exact_workspace_and_refusal():
    from fourier_feature_nets_amd import _lib, ops
    tree = complete_tree()
    scale, depth, nodes, leaves, data = tree
    starts, dirs = axis_rays(np.random.default_rng(3), 1000)
    d_color, d_alpha = upstream(1000, 3)
    plain, first = device_gradient(tree, starts, dirs, d_color, d_alpha)
    entries = first.entries
    assert entries == 2000

    def sized(max_entries):
        ws = ops.OctreeGradWorkspace()
        need = ops.octree_grad_workspace_bytes(1000, len(leaves), max_entries)
        assert need % 4 == 0
        ws.buffer = torch.empty((need // 4,), dtype=torch.float32, device="cuda")
        ws.max_entries, ws.shape = max_entries, (1000, len(leaves))
        return ws

    exact, _ = device_gradient(tree, starts, dirs, d_color, d_alpha, sized(entries))
    assert np.array_equal(bits(exact), bits(plain))
    # one entry short: refused with the documented error.  The call is made directly, since
    # ops.octree_render_volume_backward would grow the workspace and repeat it.
    ws = sized(entries - 1)
    out = torch.full((len(leaves), 4), 7.0, device="cuda")
    told = _lib.c_i64(-1)
    import ctypes
    dev = [cuda(starts), cuda(dirs), cuda(nodes, np.int64), cuda(leaves, np.int64), cuda(data),
           cuda(d_color), cuda(d_alpha)]
    with pytest.raises(_lib.FfnError, match="the workspace holds %d entries" % (entries - 1)):
        ops._call("ffn_octree_render_volume_backward",
                  *ops._walk_args(dev[0], dev[1], float(scale), depth, dev[2], dev[3]),
                  _lib.c_f(0.0), ops._dev(dev[4]), _lib.c_i(4), _lib.c_f(BG[0]), _lib.c_f(BG[1]),
                  _lib.c_f(BG[2]), _lib.c_f(0.0), ops._dev(dev[5]), ops._dev(dev[6]),
                  ops._dev(ws.buffer), _lib.c_i64(ws.buffer.numel() * 4),
                  _lib.c_i64(ws.max_entries), ops._dev(out), ctypes.byref(told))
    assert told.value == entries
    assert (out.cpu().numpy() == 7.0).all()                   # nothing was written


# (n, num_leaves, max_entries) -> bytes for plain leaves, SH degree 1, SH degree 2: what the library
# returned before the two layout tables became one.  Host arithmetic only; a change of any buffer's
# size, presence or alignment shows here without a fault.
WORKSPACE_BYTES = {
    (1, 1, 0): (1536, 2304, 2304),
    (64, 8, 1024): (52480, 50176, 56832),
    (1000, 64, 2000): (119808, 120832, 139264),
    (4096, 100000, 1 << 17): (7305216, 19981568, 30368000),
    (4097, 100001, (1 << 17) + 1): (7308288, 19984640, 30371072),
}


@pytest.mark.parametrize("shape", sorted(WORKSPACE_BYTES))
@pytest.mark.parametrize("degree", [0, 1, 2])
def test_workspace_bytes_are_the_recorded_ones(shape, degree):
    from fourier_feature_nets_amd import ops
    if degree == 0:
        got = ops.octree_grad_workspace_bytes(*shape)
    else:
        got = ops.octree_grad_sh_workspace_bytes(*shape, degree)
    assert got == WORKSPACE_BYTES[shape][degree]
