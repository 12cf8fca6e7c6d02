"""The float64 first hit of the K14 contract (include/ffn_hip.h), derived from the restatement of
the K13 walk (tests/octree_walk_reference.py) and not from any walker: of the crossings of a ray,
sorted by entry t, the first with ``leaf >= 0`` and ``t_out > t_min``; its ``max(t_in, t_min)``;
and the face of its entry plane, ``2 * axis_in + (d[axis_in] > 0 ? 0 : 1)``, or 6 when the entry
lies before ``t_min``.

A ray that enters its leaf through an edge (the two largest per-axis entry crossings coincide) has
no single entry face; ``edge_gap`` is the distance between those two crossings in t."""

import numpy as np

from tests import octree_reference as oref


def first_hit(w, scale, leaf_index, starts, directions, t_min=0.0):
    """``w``: a ``walk`` result.  -> dict with, per ray (R,): ``leaf`` (slot or -1), ``t`` (f64; 0
    on a miss), ``face`` (0 .. 5, 6 clamped, -1 miss), ``clamped``, ``crossing`` (index into the
    flat per-crossing arrays of ``w``, -1 on a miss) and ``edge_gap`` (inf on a miss)."""
    count = len(w["hit"])
    starts = np.asarray(starts, np.float32).reshape(-1, 3).astype(np.float64)
    directions = np.asarray(directions, np.float32).reshape(-1, 3).astype(np.float64)
    take = np.nonzero((w["leaf"] >= 0) & (w["t_out"] > t_min))[0]
    # the crossings are sorted by ray, then entry t: the first one taken per ray
    rays, at = np.unique(w["ray"][take], return_index=True)
    crossing = np.full(count, -1, np.int64)
    crossing[rays] = take[at]
    found = crossing >= 0
    c = crossing[found]
    leaf = np.full(count, -1, np.int64)
    leaf[found] = w["leaf"][c]
    t_in = w["t_in"][c]
    t = np.zeros(count)
    t[found] = np.maximum(t_in, t_min)
    clamped = np.zeros(count, bool)
    clamped[found] = t_in < t_min
    axis = w["axis_in"][c]
    d_axis = directions[found][np.arange(len(c)), axis]
    face = np.full(count, -1, np.int64)
    face[found] = np.where(clamped[found], 6, 2 * axis + np.where(d_axis > 0, 0, 1))
    # the leaf's own box, per axis the near crossing: how far apart are the two largest?
    centers, depths = oref.leaf_geometry(np.float32(scale), np.asarray(leaf_index, np.int64)[leaf[found]])
    half = (np.float64(np.float32(scale)) / 2.0 ** depths)[:, None]
    centers = centers.astype(np.float64)
    o, d = starts[found], directions[found]
    with np.errstate(divide="ignore", invalid="ignore"):
        near = np.minimum((centers - half - o) / d, (centers + half - o) / d)
    near = np.sort(np.where(d == 0, -np.inf, near), axis=1)
    edge_gap = np.full(count, np.inf)
    edge_gap[found] = near[:, 2] - near[:, 1]
    return dict(leaf=leaf, t=t, face=face, clamped=clamped, crossing=crossing, edge_gap=edge_gap)
