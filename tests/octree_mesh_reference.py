"""A dense numpy restatement of the K30 mesh contract (include/ffn_hip.h, ``OcTree.extract_mesh``),
written from the contract, not from the kernels.

The tree is expanded to its ``n^3`` grid of finest cells (``n = 2^(depth-1)``); nothing searches,
scans or scatters.  Solidity, masks, keys and faces are integers; offsets, colours and normals are
float64.

* opacity of a leaf: ``1 - exp(-(sigma * side))`` with the PRODUCT rounded to f32 as the kernel
  rounds it (an input of ``expm1``, not a result) and the rest in float64; 0 for a negative or NaN
  density; 1 for a tree with 3 columns or none; 1 / 0 from ``solid``;
* a cell is solid when its opacity exceeds the threshold (as an f32 value), cells outside the cube
  are empty;
* corner ``c`` has the samples ``c - 1 + (dx, dy, dz)``, bit ``4 dx + 2 dy + dz``; it is a vertex
  when the mask is neither 0 nor 255; vertices by ascending ``(i (n+1) + j)(n+1) + k``;
* faces, offsets, colours, normals as the contract states them.

BUDGETS.  ``eps = 2^-23`` (``np.finfo(np.float32).eps``, twice the unit roundoff: every count below
is therefore generous by a factor of two and no more).  Each budget is a count of f32 roundings
times ``eps`` times the magnitude of the operands.

opacity      ``a`` in [0, 1]: the product is shared, ``expm1f`` is held to 2 ulp: ``|da| <= 2 eps``.
t            ``t = N / D``, ``N = thr - a0``, ``D = a1 - a0``, ``|N| <= |D|``: ``|dN| <= 2 eps + eps``
             (one opacity, one rounding of a value <= 1), ``|dD| <= 4 eps + eps``, and the division
             rounds once (``|t| <= 1``): ``|dt| <= (3 eps + 5 eps) / |D| + eps``.
offset       a contribution ``p + t e_ax`` rounds once (magnitude <= 1): ``|dt| + eps``.  The sum of
             ``m <= 12`` contributions of magnitude <= 0.5 per component: at most 11 adds of partial
             sums <= 6, ``66 eps``; the division by ``m >= 3`` (a proper non-empty subset of a cube's
             corners is cut by at least three edges) divides that and the mean of the ``|dt|`` and
             rounds once more (magnitude <= 0.5):
             ``B_off = 8 eps / min|D| + eps + eps + 22 eps + eps = 8 eps / min|D| + 25 eps``
             in units of a cell.
position     ``center + ((c - n/2) + off) * side``: three roundings of values no larger than
             ``M = |center|_max + (n/2 + 1) side``: ``B_pos = side * B_off + 3 eps M``.
colour       a plain colour column is read, not computed.  The sum of ``m <= 8`` values of magnitude
             ``<= C``: 7 adds of partial sums <= 8 C, and the division rounds once:
             ``B_col = 57 eps C``.  An SH colour is ``1 / (1 + expf(-(k Y00)))``: the product rounds
             once (``eps |x|``, and the sigmoid's slope is <= 1/4), ``expf`` is held to 2 ulp, the
             add and the division round once each, all on values that end in (0, 1]:
             ``|ds| <= eps |x| / 4 + 4 eps``, and ``C = 1``.
normal       ``g = sum_b +-a_b``: ``8 * 2 eps`` from the opacities, 7 adds of partial sums <= 8:
             ``|dg| <= 72 eps`` per component, ``sqrt(3) * 72 eps`` in length.  ``|g|`` itself: three
             squares, two adds, one square root, each one relative rounding: ``6 eps |g|``.  The
             quotient rounds once.  ``B_n = 2 sqrt(3) 72 eps / |g| + 8 eps``.  When every opacity
             is 0 or 1 the sums are exact and a zero ``g`` is a zero normal on both sides.
"""

from collections import Counter
from typing import NamedTuple, Optional

import numpy as np

EPS = float(np.finfo(np.float32).eps)
SH_Y0 = 0.28209479177387814
PLACEMENTS = ("surface_nets", "corners")

MeshReference = NamedTuple("MeshReference", [
    ("corners", np.ndarray),        # (V,3) int64
    ("masks", np.ndarray),          # (V,) uint8
    ("triangles", np.ndarray),      # (F,3) int64
    ("offsets", np.ndarray),        # (V,3) f64, in cells
    ("vertices", np.ndarray),       # (V,3) f64
    ("colors", Optional[np.ndarray]),
    ("normals", np.ndarray),
    ("offset_budget", np.ndarray),  # (V,) in cells
    ("vertex_budget", np.ndarray),  # (V,)
    ("color_budget", float),
    ("normal_budget", np.ndarray),  # (V,)
    ("swapped_offsets", np.ndarray),    # (V,3): every t computed with its pair swapped
    ("alpha", np.ndarray),          # (L,) f64
    ("threshold", float),
    ("margin", float),              # min |alpha - threshold| over the leaves
    ("solid_cells", int),
    ("side", float),
    ("cells", int),
])


def leaf_levels_cells(leaf_index):
    """Per leaf id its level and its cell (x, y, z) on the 2^level grid."""
    ids = np.asarray(leaf_index, np.int64).copy()
    levels = np.zeros(len(ids), np.int64)
    cells = np.zeros((len(ids), 3), np.int64)
    for l, node in enumerate(ids.tolist()):
        digits = []
        while node > 0:
            digits.append((node - 1) % 8)
            node = (node - 1) // 8
        levels[l] = len(digits)
        for digit in reversed(digits):                 # root first
            cells[l] = 2 * cells[l] + [(digit >> 2) & 1, (digit >> 1) & 1, digit & 1]
    return levels, cells


def tree_depth(leaf_index):
    return int(leaf_levels_cells(leaf_index)[0].max()) + 1


def leaf_grid(leaf_index, depth):
    """-> (n,n,n) int64: per finest cell the number of the leaf that covers it, -1 for empty."""
    n = 1 << (depth - 1)
    grid = np.full((n, n, n), -1, np.int64)
    levels, cells = leaf_levels_cells(leaf_index)
    for l, (level, (x, y, z)) in enumerate(zip(levels.tolist(), cells.tolist())):
        k = 1 << (depth - 1 - level)
        block = grid[x * k:(x + 1) * k, y * k:(y + 1) * k, z * k:(z + 1) * k]
        assert (block == -1).all(), "a leaf inside another leaf"
        block[...] = l
    return grid


def opacities(leaf_data, sh_degree, num_leaves, side, alpha_threshold, solid):
    """-> alpha (L,) f64, threshold, rgb (L,3) f64 or None, the largest colour magnitude, the
    largest SH argument |k Y00| (0 for plain data)."""
    threshold = float(np.float32(alpha_threshold))
    rgb, sigma, reach = None, None, 0.0
    if leaf_data is not None:
        data = np.asarray(leaf_data).astype(np.float32)    # what the device holds
        assert data.ndim == 2 and data.shape[0] == num_leaves and data.shape[1] >= 3
        if sh_degree is not None:
            bases = (sh_degree + 1) ** 2
            assert data.shape[1] == 3 * bases + 1
            sigma = data[:, -1]
            x = data[:, [0, bases, 2 * bases]].astype(np.float64) * np.float64(np.float32(SH_Y0))
            reach = float(np.abs(x).max()) if len(x) else 0.0
            rgb = 1.0 / (1.0 + np.exp(-x))
        else:
            rgb = data[:, :3].astype(np.float64)
            if data.shape[1] >= 4:
                sigma = data[:, 3]
    if solid is not None:
        solid = np.asarray(solid)
        assert solid.dtype == bool and solid.shape == (num_leaves,)
        alpha, threshold = solid.astype(np.float64), 0.5
    elif sigma is None:
        alpha, threshold = np.ones(num_leaves), 0.5
    else:
        with np.errstate(invalid="ignore"):
            product = (sigma * np.float32(side)).astype(np.float32)      # one f32 rounding
            alpha = np.where(sigma >= 0, -np.expm1(-product.astype(np.float64)), 0.0)
    scale = 1.0 if rgb is None or sh_degree is not None else float(max(np.abs(rgb).max(), 1e-30))
    return alpha, threshold, rgb, scale, reach


def extract(scale, leaf_index, leaf_data=None, sh_degree=None, alpha_threshold=0.5,
            placement="surface_nets", center=(0.0, 0.0, 0.0), solid=None) -> MeshReference:
    """The mesh of the contract for the tree with the sorted leaf ids ``leaf_index`` (interior nodes
    are the leaves' ancestors and carry no information of their own)."""
    assert placement in PLACEMENTS
    leaf_index = np.asarray(leaf_index, np.int64)
    assert (np.diff(leaf_index) > 0).all()
    num = len(leaf_index)
    depth = tree_depth(leaf_index)
    n = 1 << (depth - 1)
    side = float(np.float32(2.0) * np.float32(scale) / np.float32(n))
    center = np.asarray([np.float32(c) for c in center], np.float64)
    alpha, thr, rgb, color_scale, sh_reach = opacities(leaf_data, sh_degree, num, side,
                                                       alpha_threshold, solid)
    leaf_solid = alpha > thr
    grid = leaf_grid(leaf_index, depth)
    padded = np.full((n + 2,) * 3, -1, np.int64)
    padded[1:-1, 1:-1, 1:-1] = grid
    # sample b of corner c is the cell c - 1 + d: index c + d of the padded grid
    samples = np.stack([padded[(b >> 2 & 1):(b >> 2 & 1) + n + 1,
                               (b >> 1 & 1):(b >> 1 & 1) + n + 1,
                               (b & 1):(b & 1) + n + 1] for b in range(8)], -1)
    inside = samples >= 0
    solid_s = inside & leaf_solid[np.maximum(samples, 0)]
    mask_grid = (solid_s.astype(np.int64) << np.arange(8)).sum(-1)
    active = (mask_grid != 0) & (mask_grid != 255)
    corners = np.argwhere(active)                       # C order: ascending key
    count = len(corners)
    masks = mask_grid[active].astype(np.uint8)
    vertex_of = np.full((n + 1,) * 3, -1, np.int64)
    vertex_of[active] = np.arange(count)
    samples = samples[active]
    solid_s = solid_s[active]
    a = np.where(samples >= 0, alpha[np.maximum(samples, 0)], 0.0)          # (V,8)

    # faces: per vertex, per axis x, y, z
    triangles = []
    for v, (c, mask) in enumerate(zip(corners.tolist(), masks.tolist())):
        for ax in range(3):
            here, below = (mask >> 7) & 1, (mask >> (7 ^ (4 >> ax))) & 1
            if here == below:
                continue
            e_u, e_v = np.eye(3, dtype=np.int64)[(ax + 1) % 3], np.eye(3, dtype=np.int64)[(ax + 2) % 3]
            quad = [np.array(c), c + e_u, c + e_u + e_v, c + e_v]
            if here:                                    # cell c is the solid one: reversed
                quad = [quad[0], quad[3], quad[2], quad[1]]
            q = [int(vertex_of[tuple(p)]) for p in quad]
            assert min(q) >= 0, "a quad corner that is not a vertex"
            triangles += [(q[0], q[1], q[2]), (q[0], q[2], q[3])]
    triangles = np.array(triangles, np.int64).reshape(-1, 3)

    # offsets: the 12 pairs, x first, then y, then z, within an axis by ascending lower bit
    offsets = np.zeros((count, 3))
    swapped = np.zeros((count, 3))
    crossings = np.zeros(count, np.int64)
    smallest = np.full(count, np.inf)
    for ax in range(3):
        step = 4 >> ax
        for b0 in range(8):
            if b0 & step:
                continue
            b1 = b0 | step
            cut = solid_s[:, b0] != solid_s[:, b1]
            p = np.array([(b0 >> 2) & 1, (b0 >> 1) & 1, b0 & 1], np.float64) - 0.5
            with np.errstate(divide="ignore", invalid="ignore"):
                t = (thr - a[:, b0]) / (a[:, b1] - a[:, b0])
                t_swapped = (thr - a[:, b1]) / (a[:, b0] - a[:, b1])
            for out, value in ((offsets, t), (swapped, t_swapped)):
                contribution = np.tile(p, (count, 1))
                contribution[:, ax] += np.where(cut, value, 0.0)
                out[cut] += contribution[cut]
            crossings += cut
            smallest = np.where(cut, np.minimum(smallest, np.abs(a[:, b1] - a[:, b0])), smallest)
    assert (crossings >= 3).all()
    offsets /= crossings[:, None]
    swapped /= crossings[:, None]
    assert (np.abs(offsets) <= 0.5).all()
    offset_budget = 8 * EPS / smallest + 25 * EPS
    if placement == "corners":
        offsets = np.zeros((count, 3))
        swapped = np.zeros((count, 3))
        offset_budget = np.zeros(count)
    vertices = center + (corners - n / 2 + offsets) * side
    reach = np.abs(center).max() + (n / 2 + 1) * side
    vertex_budget = side * offset_budget + 3 * EPS * reach

    colors, color_budget = None, 0.0
    if rgb is not None:
        picked = np.where(solid_s[..., None], rgb[np.maximum(samples, 0)], 0.0)     # (V,8,3)
        colors = picked.sum(1) / solid_s.sum(1)[:, None]
        color_budget = 57 * EPS * color_scale
        if sh_degree is not None:
            color_budget += (sh_reach / 4 + 4) * EPS

    signs = np.array([[1.0 if b & 4 else -1.0, 1.0 if b & 2 else -1.0, 1.0 if b & 1 else -1.0]
                      for b in range(8)])
    g = (a[..., None] * signs).sum(1)
    length = np.sqrt((g * g).sum(1))
    with np.errstate(divide="ignore", invalid="ignore"):
        normals = np.where(length[:, None] > 0, -g / length[:, None], 0.0)
        normal_budget = np.where(length > 0, 2 * np.sqrt(3) * 72 * EPS / length + 8 * EPS, 0.0)

    return MeshReference(corners, masks, triangles, offsets, vertices, colors, normals,
                         offset_budget, vertex_budget, color_budget, normal_budget, swapped,
                         alpha, thr, float(np.abs(alpha - thr).min()),
                         int(leaf_solid[grid[grid >= 0]].sum()), side, n)


# ------------------------------------------------------------------------------ invariants
def edges_pair_up(triangles) -> bool:
    """Every directed edge occurs as often as its reverse: closed and consistently oriented."""
    tri = np.asarray(triangles, np.int64)
    edges = Counter()
    for a, b in ((0, 1), (1, 2), (2, 0)):
        edges.update(zip(tri[:, a].tolist(), tri[:, b].tolist()))
    return all(edges.get((v, u), 0) == k for (u, v), k in edges.items())


def six_volumes(points, triangles):
    """Six times the signed volume: the sum of det(p0, p1, p2).  Exact for integer points."""
    p = np.asarray(points)
    p = p.astype(np.int64) if np.issubdtype(p.dtype, np.integer) else p.astype(np.float64)
    tri = np.asarray(triangles, np.int64)
    p0, p1, p2 = p[tri[:, 0]], p[tri[:, 1]], p[tri[:, 2]]
    return (p0 * np.cross(p1, p2)).sum()


def euler_characteristic(num_vertices, triangles) -> int:
    tri = np.asarray(triangles, np.int64)
    edges = set()
    for a, b in ((0, 1), (1, 2), (2, 0)):
        lo, hi = np.minimum(tri[:, a], tri[:, b]), np.maximum(tri[:, a], tri[:, b])
        edges.update(zip(lo.tolist(), hi.tolist()))
    return int(num_vertices) - len(edges) + len(tri)
