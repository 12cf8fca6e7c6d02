"""K25 restated in numpy float32: an octree's leaves rasterised into the K9 occupancy bits.

The kernel (csrc/occupancy.hip, ``ffn_occupancy_from_octree``) must reproduce ``Rule().words``
bit for bit.  Every step is one rounded f32 operation, in the order written here.

* Leaf ``l`` with id ``leaf_index[l]``: centre ``c`` and depth ``d`` from
  ``octree_reference.leaf_geometry``, ``h = scale * 2^-d`` (exact).  Per axis
  ``lo = fl(fl(c - h) + center)``, ``hi = fl(fl(c + h) + center)``.
* Grid coordinate ``f(x) = fl(fl(x - box_min) * inv)``, ``inv = fl((float)G / box_size)``: what
  ``occupied_at`` (csrc/occupancy_map.h) truncates for a sample at ``x``.
* Per axis the leaf covers the half-open interval ``[f(lo), f(hi))`` and marks every cell
  ``[i, i + 1)`` that meets it: ``i0 = clamp(floor(f(lo)), 0, G - 1)``,
  ``i1 = max(i0, clamp(ceil(f(hi)) - 1, 0, G - 1))``.  A leaf with ``f(hi) <= 0`` or
  ``f(lo) >= G`` on any axis lies outside and marks nothing.
* With a threshold a leaf whose density ``<= sigma_threshold`` marks nothing; NaN marks.
* Row ``(iy, iz)`` of a leaf is the run of bits ``(iz G + iy) G + ix0 .. + ix1``, ORed in word by
  word with one mask per word.

The guarantee: ``f`` is monotone (an f32 subtraction of a constant, an f32 multiplication by a
positive constant), so every f32 point ``p`` with ``f(lo) <= f(p) < f(hi)`` on all three axes, for a
leaf that marks, has ``floor(f(p))`` inside ``[i0, i1]`` after the clamp and is reported occupied
by ``occupied_at``.  ``promised`` selects those points, ``occupied_at`` restates the lookup.

``Rule`` keeps each decision in a method of its own, so that a test can override one of them (a
mutant) and require that its inputs notice."""

import numpy as np

from tests import octree_reference as oref

F = np.float32


def grid_inv(box_size, resolution):
    """``make_map``: cells per world unit, one f32 division per axis."""
    return (F(resolution) / np.asarray(box_size, F)).astype(F)


def grid_coord(x, box_min, inv):
    """f(x) per axis for x (..., 3)."""
    return ((np.asarray(x, F) - np.asarray(box_min, F)).astype(F) * np.asarray(inv, F)).astype(F)


def occupied_at(words, points, box_min, box_size, resolution):
    """The K9 lookup for points (N,3) f32 -> bool (N,)."""
    g = int(resolution)
    f = grid_coord(points, box_min, grid_inv(box_size, g))
    nan = np.isnan(f).any(1)
    idx = np.minimum(np.maximum(np.where(np.isnan(f), F(0), f), F(0)), F(g - 1)).astype(np.int64)
    cell = (idx[:, 2] * g + idx[:, 1]) * g + idx[:, 0]
    bit = (np.asarray(words, np.uint32)[cell >> 5] >> (cell & 31).astype(np.uint32)) & 1
    return nan | (bit != 0)


def num_words(resolution):
    return (int(resolution) ** 3 + 31) // 32


def cells_of(words, resolution):
    """The set cells of a word array as a bool (G,G,G) array indexed [iz, iy, ix]."""
    g = int(resolution)
    bits = (np.asarray(words, np.uint32)[:, None] >> np.arange(32, dtype=np.uint32)) & 1
    return bits.reshape(-1)[:g ** 3].reshape(g, g, g).astype(bool)


def words_of(cells):
    """The inverse of ``cells_of``."""
    cells = np.asarray(cells, bool)
    flat = cells.reshape(-1)
    padded = np.zeros(num_words(cells.shape[0]) * 32, np.uint64)
    padded[:len(flat)] = flat
    return (padded.reshape(-1, 32) << np.arange(32, dtype=np.uint64)).sum(1).astype(np.uint32)


def dilate_cells(cells):
    """One pass of the 26-neighbourhood (K9b) on a bool (G,G,G) array."""
    g = cells.shape[0]
    padded = np.zeros((g + 2,) * 3, bool)
    padded[1:-1, 1:-1, 1:-1] = cells
    out = np.zeros_like(cells)
    for dz in range(3):
        for dy in range(3):
            for dx in range(3):
                out |= padded[dz:dz + g, dy:dy + g, dx:dx + g]
    return out


class Rule:
    """The rule, one decision per method."""

    def world_box(self, scale, center, leaf_index):
        """-> lo, hi (L,3) f32."""
        centers, depths = oref.leaf_geometry(F(scale), np.asarray(leaf_index, np.int64))
        h = (F(scale) * np.ldexp(F(1), -depths.astype(np.int64)).astype(F)).astype(F)[:, None]
        o = np.asarray(center, F)
        lo = ((centers - h).astype(F) + o).astype(F)
        hi = ((centers + h).astype(F) + o).astype(F)
        return lo, hi

    def outside(self, f_lo, f_hi, g):
        """Per leaf and axis: the interval does not meet [0, G)."""
        return (f_hi <= F(0)) | (f_lo >= F(g))

    def first_index(self, f_lo, g):
        return np.minimum(np.maximum(np.floor(f_lo), F(0)), F(g - 1)).astype(np.int64)

    def last_index(self, f_hi, g):
        return np.minimum(np.maximum((np.ceil(f_hi) - F(1)).astype(F), F(0)), F(g - 1)).astype(np.int64)

    def empty(self, density, sigma_threshold):
        """Per leaf: the threshold rule.  NaN <= t is false: a NaN density marks."""
        with np.errstate(invalid="ignore"):
            return np.asarray(density, F) <= F(sigma_threshold)

    def run_masks(self, begin, end):
        """Runs of bits begin..end (inclusive, int64 arrays (R,)) -> (word, mask) arrays, one
        entry per touched word."""
        w0, w1 = begin >> 5, end >> 5
        words, masks = [], []
        for k in range(int((w1 - w0).max()) + 1 if len(begin) else 0):
            w = w0 + k
            live = w <= w1
            first = np.where(w == w0, begin & 31, 0).astype(np.uint64)
            last = np.where(w == w1, end & 31, 31).astype(np.uint64)
            mask = (np.uint64(0xffffffff) >> (np.uint64(31) - last)) & \
                   ((np.uint64(0xffffffff) << first) & np.uint64(0xffffffff))
            words.append(w[live])
            masks.append(mask[live].astype(np.uint32))
        if not words:
            return np.zeros(0, np.int64), np.zeros(0, np.uint32)
        return np.concatenate(words), np.concatenate(masks)

    def plan(self, leaf_index, scale, center, box_min, box_size, resolution, density=None,
             sigma_threshold=None):
        """-> marks (L,) bool, i0, i1 (L,3) int64 [x, y, z], f_lo, f_hi (L,3) f32."""
        g = int(resolution)
        lo, hi = self.world_box(scale, center, leaf_index)
        inv = grid_inv(box_size, g)
        f_lo, f_hi = grid_coord(lo, box_min, inv), grid_coord(hi, box_min, inv)
        marks = ~self.outside(f_lo, f_hi, g).any(1)
        if sigma_threshold is not None:
            marks &= ~self.empty(density, sigma_threshold)
        i0 = self.first_index(f_lo, g)
        i1 = np.maximum(i0, self.last_index(f_hi, g))
        return marks, i0, i1, f_lo, f_hi

    def rows(self, marks, i0, i1):
        """Rows per leaf: ny nz, 0 for a leaf that marks nothing."""
        n = i1 - i0 + 1
        return np.where(marks, n[:, 1] * n[:, 2], 0)

    def words(self, leaf_index, scale, center, box_min, box_size, resolution, density=None,
              sigma_threshold=None, dilate=0, into=None):
        """-> the grid's uint32 words.  ``into``: words to fold into (not modified)."""
        g = int(resolution)
        marks, i0, i1, _, _ = self.plan(leaf_index, scale, center, box_min, box_size, g, density,
                                        sigma_threshold)
        rows = self.rows(marks, i0, i1)
        leaf = np.repeat(np.arange(len(rows)), rows)
        local = np.arange(rows.sum()) - np.repeat(np.cumsum(rows) - rows, rows)
        ny = (i1 - i0 + 1)[leaf, 1]
        iy, iz = i0[leaf, 1] + local % ny, i0[leaf, 2] + local // ny
        begin = (iz * g + iy) * g + i0[leaf, 0]
        end = begin + (i1 - i0)[leaf, 0]
        word, mask = self.run_masks(begin, end)
        out = np.zeros(num_words(g), np.uint32)
        np.bitwise_or.at(out, word, mask)
        if dilate:
            cells = cells_of(out, g)
            for _ in range(int(dilate)):
                cells = dilate_cells(cells)
            out = words_of(cells)
        if into is not None:
            out = out | np.asarray(into, np.uint32)
        return out


def promised(rule, points, leaf_of_point, marks, f_lo, f_hi, box_min, box_size, resolution):
    """Which of points (N,3) f32, each belonging to leaf ``leaf_of_point``, the guarantee covers:
    the leaf marks, and ``f(lo) <= f(p) < f(hi)`` on all three axes."""
    f = grid_coord(points, box_min, grid_inv(box_size, resolution))
    inside = ((f >= f_lo[leaf_of_point]) & (f < f_hi[leaf_of_point])).all(1)
    return inside & marks[leaf_of_point]


def leaf_points(lo, hi, rng, per_leaf=4):
    """Points inside the leaves' world boxes: random interior points, ``lo``,
    ``nextafter(lo -> hi)`` and ``nextafter(hi -> lo)`` -> points (N,3) f32, leaf (N,)."""
    count = len(lo)
    u = rng.random((per_leaf, count, 3)).astype(F)
    inner = (lo[None] + (u * (hi - lo)[None]).astype(F)).astype(F)
    inner = np.minimum(np.maximum(inner, lo[None]), hi[None])
    pts = np.concatenate([inner.reshape(-1, 3), lo, np.nextafter(lo, hi), np.nextafter(hi, lo)])
    leaf = np.concatenate([np.tile(np.arange(count), per_leaf)] + [np.arange(count)] * 3)
    return pts.astype(F), leaf
