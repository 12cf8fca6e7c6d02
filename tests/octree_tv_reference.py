"""A float64 / pure-Python restatement of the K20 contract (include/ffn_hip.h): the face adjacency
of a sparse octree from its ids alone, the edge list, the Charbonnier total-variation energy and its
gradient.  Nothing here runs on a GPU or reads a file.

ADJACENCY.  A leaf's id gives its level ``d`` and its cell ``(ix, iy, iz)`` on the ``2^d`` grid (child
index ``4 [x] + 2 [y] + [z]``).  Across a face: one cell along the axis; outside ``[0, 2^d)`` -> -1;
otherwise descend from the root along that cell's path (``id = 8 id + 1 + child``): an id among the
leaves answers with that leaf's number, an id that is neither leaf nor node is empty (-1), and an id
that is still a node at level ``d`` means finer leaves on the other side (-1).  ``(i, dir)`` is an
EDGE when ``j = nb(i, dir) >= 0`` and (``level(j) < level(i)`` or ``dir`` is a + direction); edges
are numbered in ``(i, dir)`` order.

ENERGY.  ``R(v) = (1/E) sum_e sum_c lambda_c (sqrt(d^2 + eps^2) - eps)``, ``d = v[i,c] - v[j,c]``;
``dR/dv[i,c] += (lambda_c / E) d / sqrt(d^2 + eps^2)`` and ``dR/dv[j,c] -=`` the same.  The inputs are
the float32 values the kernel reads (rows, lambda, eps), the arithmetic float64.

BUDGET, derived, not tuned to the kernel; ``u = 2^-24`` is one relative f32 rounding step.  The kernel
computes ``d = a - b`` (1 step), ``s = sqrtf(fmaf(d, d, eps * eps))`` -- ``s`` moves by at most ``u``
relative through ``d`` (``|d ds/dd| = d^2/s^2 <= 1``), by ``u/2`` each for the rounding of ``eps *
eps`` and of the fma (the square root halves them) and by ``u`` for the square root itself: 3 steps
-- ``scale_c = lambda_c / (float)E`` (the conversion and the division: 2 steps), the derivative ``(d
/ s) * scale_c`` (``d``: 1, ``s``: 3, the division: 1, ``scale_c``: 2, the product: 1) and the term
``(s - eps) * scale_c`` (the subtraction cancels: ``s``'s 3 steps stay ABSOLUTE, ``3 u s``; then the
subtraction 1, ``scale_c`` 2, the product 1, relative to the term):

    b(derivative) = 8 u |derivative|
    b(term)       = scale_c (3 u s + 4 u (s - eps))

each plus ``2^-126`` for a result in the subnormal range.  A leaf's row is the f32 sum of its ``m``
signed derivatives in some order: ``+ m u sum |derivative|`` (``+ u |prior| + u |result|`` for the one
add of ``accumulate`` is the caller's).  The energy is the f32 sum of its ``M`` non-zero-weight terms
in some order: ``+ M u sum |term|``."""

import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126
DIRECTIONS = ((0, -1), (0, 1), (1, -1), (1, 1), (2, -1), (2, 1))     # -x +x -y +y -z +z


def decode(leaf_id):
    """id -> (level, ix, iy, iz)."""
    digits = []
    node = int(leaf_id)
    while node > 0:
        digits.append((node - 1) % 8)
        node = (node - 1) // 8
    cell = [0, 0, 0]
    for child in reversed(digits):
        cell = [2 * cell[0] + (child >> 2 & 1), 2 * cell[1] + (child >> 1 & 1),
                2 * cell[2] + (child & 1)]
    return len(digits), cell[0], cell[1], cell[2]


def neighbors(node_index, leaf_index):
    """-> (L,6) int64, from dictionaries of the ids alone."""
    leaf_number = {int(v): k for k, v in enumerate(np.asarray(leaf_index).tolist())}
    nodes = set(int(v) for v in np.asarray(node_index).tolist())
    out = np.full((len(leaf_number), 6), -1, np.int64)
    for leaf_id, number in leaf_number.items():
        level, ix, iy, iz = decode(leaf_id)
        for k, (axis, step) in enumerate(DIRECTIONS):
            cell = [ix, iy, iz]
            cell[axis] += step
            if not 0 <= cell[axis] < (1 << level):
                continue
            node = 0
            for bit in range(level - 1, -1, -1):
                child = 4 * (cell[0] >> bit & 1) + 2 * (cell[1] >> bit & 1) + (cell[2] >> bit & 1)
                node = 8 * node + 1 + child
                if node in leaf_number:
                    out[number, k] = leaf_number[node]
                    break
                if node not in nodes:
                    break
    return out


def levels(leaf_index):
    return np.array([decode(v)[0] for v in np.asarray(leaf_index).tolist()], np.int64)


def edges(nb, level):
    """-> (E,2) int64 rows (i, j) in (i, dir) order."""
    out = []
    for i in range(len(nb)):
        for k in range(6):
            j = int(nb[i, k])
            if j >= 0 and (level[j] < level[i] or k % 2 == 1):
                out.append((i, j))
    return np.array(out, np.int64).reshape(-1, 2)


def tree_edges(node_index, leaf_index):
    nb = neighbors(node_index, leaf_index)
    return nb, edges(nb, levels(leaf_index))


def energy(rows, edge_list, lam, eps):
    """float64 R of float64 ``rows`` (used for central differences too)."""
    count = len(edge_list)
    if count == 0:
        return 0.0
    d = rows[edge_list[:, 0]] - rows[edge_list[:, 1]]
    return float(((np.sqrt(d * d + eps * eps) - eps) * lam[None, :]).sum() / count)


def total_variation(rows, edge_list, lam, eps):
    """rows (L, stride), lam (stride,), eps: the float32 values the kernel reads.  -> dict: ``value``,
    ``value_budget``, ``grad`` (L, stride) f64, ``budget`` (L, stride), ``incidences`` (L,)."""
    rows = np.asarray(rows, np.float32).astype(np.float64)
    lam = np.asarray(lam, np.float32).astype(np.float64)
    eps = float(np.float32(eps))
    leaves, stride = rows.shape
    count = len(edge_list)
    grad = np.zeros((leaves, stride))
    budget = np.zeros((leaves, stride))
    incidences = np.zeros(leaves, np.int64)
    if count == 0:
        return dict(value=0.0, value_budget=0.0, grad=grad, budget=budget, incidences=incidences)
    i, j = edge_list[:, 0], edge_list[:, 1]
    scale = lam / count
    d = rows[i] - rows[j]
    s = np.sqrt(d * d + eps * eps)
    term = (s - eps) * scale[None, :]
    deriv = d / s * scale[None, :]
    live = (lam > 0)[None, :]
    b_term = np.where(live, scale[None, :] * (3 * U * s + 4 * U * (s - eps)) + TINY, 0.0)
    b_deriv = np.where(live, 8 * U * np.abs(deriv) + TINY, 0.0)
    total = np.zeros((leaves, stride))
    for end, sign in ((i, 1.0), (j, -1.0)):
        np.add.at(grad, end, sign * deriv)
        np.add.at(budget, end, b_deriv)
        np.add.at(total, end, np.abs(deriv))
        np.add.at(incidences, end, 1)
    budget += incidences[:, None] * U * total
    terms = count * int((lam > 0).sum())
    return dict(value=float(term.sum()), value_budget=float(b_term.sum() + terms * U * np.abs(term).sum()),
                grad=grad, budget=budget, incidences=incidences)


def boxes(leaf_index, depth_levels):
    """Integer boxes ``[lo, hi)`` per leaf on the ``2^depth_levels`` grid: (L,3) lo, (L,3) hi."""
    lo, hi = [], []
    for v in np.asarray(leaf_index).tolist():
        level, ix, iy, iz = decode(v)
        side = 1 << (depth_levels - level)
        lo.append((ix * side, iy * side, iz * side))
        hi.append(((ix + 1) * side, (iy + 1) * side, (iz + 1) * side))
    return np.array(lo, np.int64).reshape(-1, 3), np.array(hi, np.int64).reshape(-1, 3)


def touching_pairs(leaf_index):
    """Every unordered pair of leaves whose boxes share a piece of a face of positive area, by brute
    force on the integer boxes.  -> a set of (min, max) leaf numbers."""
    level = levels(leaf_index)
    lo, hi = boxes(leaf_index, int(level.max()) if len(level) else 0)
    pairs = set()
    for a in range(len(lo)):
        overlap = np.minimum(hi[a], hi) - np.maximum(lo[a], lo)          # (L,3)
        for axis in range(3):
            others = [k for k in range(3) if k != axis]
            meet = (hi[a, axis] == lo[:, axis]) | (lo[a, axis] == hi[:, axis])
            face = meet & (overlap[:, others[0]] > 0) & (overlap[:, others[1]] > 0)
            for b in np.nonzero(face)[0]:
                pairs.add((min(a, int(b)), max(a, int(b))))
    return pairs
