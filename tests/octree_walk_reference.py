"""A float64 restatement of the K13 ray walk, written from its contract (include/ffn_hip.h), not
from the reference's ``_trace_ray_path``:

* a REGION is a leaf, or a maximal empty cell (a child slot of an interior node that is in
  neither index).  Its box is ``c +- h`` with ``c`` the f32 chain centre
  (``tests/octree_reference.py``; exact in float64) and ``h = scale / 2^level``;
* every region is slab-tested against every ray in float64; the regions a ray crosses are those
  with ``t_exit > t_entry``, ordered by entry t;
* a zero direction component constrains nothing when the start lies inside the slab and misses
  otherwise.  "Inside" is ``lo <= o < hi``, the side the ``>=`` child rule takes, and
  ``o == scale`` on the cube's own face;
* ``path`` cuts the list to the ``max_length - 1`` rule and fills with the cube's exit t and -1;
  ``spans`` is the first entry / last exit over the leaves of the same list.

Nothing here walks: there is no order of visits to get wrong.  The enumeration is pruned through
the tree (a child is tested only if the ray comes within ``PRUNE`` of its box), which drops only
regions far from the ray.

Per ray it also reports the MARGIN: the smallest ``|t_exit - t_entry|`` over all regions that
were tested, the near misses (negative chords) included.  A ray whose margin is below the
rounding of the arithmetic under test has no single right answer: an implementation may or may
not see the sliver.  ``budgets`` gives that rounding from operand magnitudes."""

import numpy as np

from tests import octree_reference as oref

PRUNE = 1e-3        # in units of the root scale


def regions(scale, node_index, leaf_index):
    """-> ids (M,), slot (M,) index into leaf_index or -1, centres (M,3) f64, half (M,) f64."""
    scale = np.float32(scale)
    node_index = np.asarray(node_index, np.int64)
    leaf_index = np.asarray(leaf_index, np.int64)
    if len(node_index) == 0:
        ids = leaf_index[:1].copy()
    else:
        children = (8 * node_index[:, None] + 1 + np.arange(8)[None, :]).ravel()
        ids = children[~np.isin(children, node_index)]
    at = np.searchsorted(leaf_index, ids)
    is_leaf = leaf_index[np.minimum(at, len(leaf_index) - 1)] == ids
    slot = np.where(is_leaf, at, -1).astype(np.int64)
    centers, depths = oref.leaf_geometry(scale, ids)
    half = np.float64(scale) / 2.0 ** depths
    return ids, slot, centers.astype(np.float64), half


def _slab(o, d, lo, hi, top, zero_rule="lower"):
    """Per row: entry t, exit t, and per axis the near / far crossing.  o, d, lo, hi: (K,3).
    ``zero_rule``: see ``walk``."""
    with np.errstate(divide="ignore", invalid="ignore"):
        t0 = (lo - o) / d
        t1 = (hi - o) / d
    near, far = np.minimum(t0, t1), np.maximum(t0, t1)
    zero = d == 0
    if zero_rule == "lower":
        inside = (o >= lo) & ((o < hi) | ((o == top) & (hi >= top * (1 - 1e-6))))
    else:
        inside = ((o > lo) | ((o == -top) & (lo <= -top * (1 - 1e-6)))) & (o <= hi)
    near = np.where(zero, np.where(inside, -np.inf, np.inf), near)
    far = np.where(zero, np.where(inside, np.inf, -np.inf), far)
    return near, far


def walk(scale, node_index, leaf_index, starts, directions, chunk=8192, zero_rule="lower"):
    """``zero_rule``: which side of a plane a zero direction component belongs to.  "lower" is the
    contract (``lo <= o < hi``); "upper" (``lo < o <= hi``) is a deliberately WRONG restatement
    that tests/test_octree_lattice_gpu.py holds its checkers against.

    -> dict with, per ray (R,): ``hit`` (crosses the cube with a chord of positive length),
    ``root_in`` / ``root_out`` (the cube's entry / exit t), ``margin``, ``offsets`` (R+1,) into
    the flat per-crossing arrays, sorted by ray and entry t: ``t_in``, ``t_out``, ``leaf`` (slot
    or -1), ``axis_in`` / ``axis_out`` (the axes whose planes give the entry / exit)."""
    scale32 = np.float32(scale)
    scale = np.float64(scale32)
    node_index = np.asarray(node_index, np.int64)
    leaf_index = np.asarray(leaf_index, np.int64)
    starts = np.asarray(starts, np.float32).reshape(-1, 3).astype(np.float64)
    directions = np.asarray(directions, np.float32).reshape(-1, 3).astype(np.float64)
    count = len(starts)
    near, far = _slab(starts, directions, np.full_like(starts, -scale), np.full_like(starts, scale),
                      scale, zero_rule)
    root_in, root_out = near.max(1), far.min(1)
    finite = np.isfinite(starts).all(1) & np.isfinite(directions).all(1)
    with np.errstate(invalid="ignore"):
        hit = finite & (root_in < root_out) & np.isfinite(root_in) & np.isfinite(root_out)
    margin = np.full(count, np.inf)
    found = []
    for begin in range(0, count, chunk):
        rays = np.nonzero(hit[begin:begin + chunk])[0] + begin
        ids = np.zeros(len(rays), np.int64)
        centers = np.zeros((len(rays), 3), np.float32)
        level = 0
        while len(rays):
            half32 = np.float32(scale32 / np.float32(2 ** level))
            interior = np.isin(ids, node_index)
            # regions at this level: the exact test
            r, c = rays[~interior], centers[~interior].astype(np.float64)
            if len(r):
                near, far = _slab(starts[r], directions[r], c - np.float64(half32),
                                  c + np.float64(half32), scale, zero_rule)
                t_in, t_out = near.max(1), far.min(1)
                with np.errstate(invalid="ignore"):
                    chord = t_out - t_in
                    np.minimum.at(margin, r, np.where(np.isnan(chord), np.inf, np.abs(chord)))
                    keep = chord > 0
                rid = ids[~interior][keep]
                at = np.searchsorted(leaf_index, rid)
                is_leaf = leaf_index[np.minimum(at, len(leaf_index) - 1)] == rid
                found.append((r[keep], t_in[keep], t_out[keep], np.where(is_leaf, at, -1),
                              near[keep].argmax(1), far[keep].argmin(1)))
            # interior nodes: their eight children, kept if the ray comes near the child's box
            r, i, c = rays[interior], ids[interior], centers[interior]
            if len(r) == 0:
                break
            child_half = np.float32(half32 / np.float32(2))
            digit = np.arange(8)
            sign = np.stack([(digit & 4) > 0, (digit & 2) > 0, (digit & 1) > 0], 1)      # (8,3)
            child_c = np.where(sign[None], c[:, None, :] + child_half,
                               c[:, None, :] - child_half).astype(np.float32).reshape(-1, 3)
            child_i = (8 * i[:, None] + 1 + digit[None]).ravel()
            child_r = np.repeat(r, 8)
            grow = np.float64(child_half) + PRUNE * scale
            c64 = child_c.astype(np.float64)
            near, far = _slab(starts[child_r], directions[child_r], c64 - grow, c64 + grow, np.inf,
                              zero_rule)
            with np.errstate(invalid="ignore"):
                keep = near.max(1) <= far.min(1)
            rays, ids, centers = child_r[keep], child_i[keep], child_c[keep]
            level += 1
    if found:
        ray, t_in, t_out, leaf, axis_in, axis_out = [np.concatenate(x) for x in zip(*found)]
    else:
        ray = leaf = axis_in = axis_out = np.zeros(0, np.int64)
        t_in = t_out = np.zeros(0)
    order = np.lexsort((t_out, t_in, ray))
    ray = ray[order]
    offsets = np.searchsorted(ray, np.arange(count + 1))
    return dict(hit=hit, root_in=root_in, root_out=root_out, margin=margin, offsets=offsets,
                ray=ray, t_in=t_in[order], t_out=t_out[order], leaf=leaf[order].astype(np.int64),
                axis_in=axis_in[order], axis_out=axis_out[order])


def path(w, max_length):
    """The ``Path`` arrays of a ``walk`` result: t_stops (R,L) f64, leaves (R,L) int64, and
    ``written`` (R,) the number of stops.  Rows of rays that miss hold NaN / -1."""
    count = len(w["hit"])
    written = np.minimum(np.diff(w["offsets"]), max_length - 1)
    t_stops = np.repeat(np.where(w["hit"], w["root_out"], np.nan)[:, None], max_length, 1)
    leaves = np.full((count, max_length), -1, np.int64)
    k = np.arange(len(w["ray"])) - w["offsets"][w["ray"]]
    keep = k < max_length - 1
    t_stops[w["ray"][keep], k[keep]] = w["t_in"][keep]
    leaves[w["ray"][keep], k[keep]] = w["leaf"][keep]
    return t_stops, leaves, written


def spans(w, scale, depth, directions, t_min=0.0, pad=1.0):
    """-> t_in, t_out (f64; 0 without a hit), hit: over the leaves that end after ``t_min``,
    ``max(first entry, t_min) - width`` and ``last exit + width``, width = ``pad`` finest-cell
    sides (2 scale / 2^(depth-1)) along the ray, in t."""
    count = len(w["hit"])
    directions = np.asarray(directions, np.float32).reshape(-1, 3).astype(np.float64)
    take = (w["leaf"] >= 0) & (w["t_out"] > t_min)
    first = np.full(count, np.inf)
    last = np.full(count, -np.inf)
    np.minimum.at(first, w["ray"][take], np.maximum(w["t_in"][take], t_min))
    np.maximum.at(last, w["ray"][take], w["t_out"][take])
    hit = np.isfinite(first)
    with np.errstate(divide="ignore", invalid="ignore"):
        width = pad * (2.0 * np.float64(np.float32(scale)) / 2 ** (depth - 1)) / np.linalg.norm(directions, axis=1)
    return np.where(hit, first - width, 0.0), np.where(hit, last + width, 0.0), hit


def _ulp(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def budgets(w, scale, starts, directions):
    """f32 rounding of a plane crossing ``(plane - o) / d``, from operand magnitudes: the plane
    ``c +- h`` is rounded to f32 (half an ulp of |plane|), the difference once more (half an ulp
    of at most |plane| + |o|), the quotient once (half an ulp of t); the cell of an entry point
    ``o + t d`` adds roundings of the same operands.  Allowed: ``4 (ulp(|plane| + |o|) / |d| +
    ulp(t))`` on the crossing's own axis.

    -> per crossing ``entry`` and ``exit`` budgets, and per ray the largest of them (``ray``;
    0 for rays without a crossing)."""
    scale = np.float64(np.float32(scale))
    starts = np.asarray(starts, np.float32).reshape(-1, 3).astype(np.float64)
    directions = np.asarray(directions, np.float32).reshape(-1, 3).astype(np.float64)

    def one(t, axis):
        o = starts[w["ray"], axis]
        d = directions[w["ray"], axis]
        plane = o + t * d
        with np.errstate(divide="ignore", invalid="ignore"):
            return 4 * (_ulp(np.abs(plane) + np.abs(o)) / np.abs(d) + _ulp(t))

    entry, exit_ = one(w["t_in"], w["axis_in"]), one(w["t_out"], w["axis_out"])
    per_ray = np.zeros(len(w["hit"]))
    np.maximum.at(per_ray, w["ray"], np.maximum(entry, exit_))
    return entry, exit_, per_ray
