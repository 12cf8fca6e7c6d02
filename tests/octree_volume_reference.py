"""A float64 restatement of the K15 volume render, written from its contract (include/ffn_hip.h)
on the per-crossing arrays of ``tests/octree_walk_reference.walk`` (``ray``, ``t_in``, ``t_out``,
``leaf``).  Nothing here walks: the crossings of a ray are already there, sorted by entry t.

Of the crossings of a ray those with ``leaf >= 0`` and ``t_out > t_min`` are TAKEN, in order, until
the transmittance is at or below ``min_transmittance``:

    t0 = max(t_in, t_min);  L = (t_out - t0) |d|;  sigma = max(data[leaf, 3], 0)  (NaN -> 0)
    a = 1 - exp(-sigma L);  w = T a;  C += w rgb;  T *= 1 - a
    depth = the t0 of the largest w (the first of equals; 0 when no w > 0)
    colour = C + T background;  alpha = 1 - T

The BUDGET of a ray is derived, not tuned to the kernel:

    budget_c = cmax * sum_k sigma_k (entry_k + exit_k) |d|
               + 8 (n + 1) 2^-24 max(1, cmax, |bg|)

``entry_k`` / ``exit_k`` are the f32 roundings of the two plane crossings of taken leaf k
(``octree_walk_reference.budgets``) and ``cmax`` the largest ``|rgb|`` in the data.  First term:
with ``sum w <= 1``, changing the optical depth of one segment by ``dx`` moves the colour by at
most ``cmax dx`` (``|d/dx exp(-x)| <= 1``).  Second term: at most eight f32 roundings per leaf step
(the chord, its scaling by the norm, the optical depth, ``expf`` within 2 ulp, ``1 - e`` with an
absolute error of one ulp of 1, the weight, the product with the colour, the sum) on values of at
most that magnitude, and one more step for ``C + T bg``.  The alpha budget is the same expression
with ``cmax = 1`` and no background."""

import numpy as np

from tests import octree_walk_reference as wref

EPS = 2.0 ** -24


def composite(w, scale, starts, directions, leaf_data, t_min=0.0, background=(0.0, 0.0, 0.0),
              min_transmittance=0.0):
    """``w``: a ``walk`` result; ``leaf_data`` (L, C >= 4).  -> dict with, per ray (R,): ``color``
    (R,3), ``alpha``, ``depth``, ``trans`` (the final T), ``count`` (leaf crossings taken),
    ``gap`` (largest weight minus the second largest; the largest when there is one, 0 for none),
    ``budget_c``, ``budget_a``, ``clamped`` (the depth is ``t_min`` itself), ``best`` (index into
    ``taken`` of the depth's crossing, -1 for none); and per taken crossing (K,): ``taken`` (index
    into the flat arrays of ``w``), ``weights``, ``t0`` and ``entry`` (the budget of ``t0``)."""
    count = len(w["hit"])
    data = np.asarray(leaf_data).astype(np.float64)      # f32 as the kernel reads it, or f64
    bg = np.asarray(background, np.float32).astype(np.float64)
    directions = np.asarray(directions, np.float32).reshape(-1, 3).astype(np.float64)
    norm = np.linalg.norm(directions, axis=1)
    entry, exit_, _ = wref.budgets(w, scale, starts, directions)
    cmax = float(np.abs(data[:, :3]).max())

    with np.errstate(invalid="ignore"):
        qualifies = np.nonzero((w["leaf"] >= 0) & (w["t_out"] > t_min))[0]
    ray = w["ray"][qualifies]
    # position of each qualifying crossing among its ray's (the arrays are sorted by ray, entry t)
    first_of_ray = np.searchsorted(ray, np.arange(count))
    rank = np.arange(len(ray)) - first_of_ray[ray]

    trans = np.ones(count)
    color = np.zeros((count, 3))
    w_best = np.zeros(count)
    second = np.zeros(count)
    depth = np.zeros(count)
    best = np.full(count, -1, np.int64)
    clamped = np.zeros(count, bool)
    taken_n = np.zeros(count, np.int64)
    drift = np.zeros(count)
    alive = np.ones(count, bool)
    taken, weights, t0s, base = [], [], [], 0
    for k in range(int(rank.max()) + 1 if len(rank) else 0):
        rows = np.nonzero(rank == k)[0]
        rows = rows[alive[ray[rows]]]
        if len(rows) == 0:
            break
        r, c = ray[rows], qualifies[rows]
        t0 = np.maximum(w["t_in"][c], t_min)
        length = (w["t_out"][c] - t0) * norm[r]
        sigma = data[w["leaf"][c], 3]
        sigma = np.where(sigma > 0, sigma, 0.0)               # NaN and negatives: 0
        a = 1.0 - np.exp(-(sigma * length))
        weight = trans[r] * a
        color[r] += weight[:, None] * data[w["leaf"][c], :3]
        better = weight > w_best[r]
        second[r] = np.where(better, w_best[r], np.maximum(second[r], weight))
        w_best[r] = np.where(better, weight, w_best[r])
        depth[r] = np.where(better, t0, depth[r])
        clamped[r] = np.where(better, w["t_in"][c] < t_min, clamped[r])
        best[r] = np.where(better, base + np.arange(len(rows)), best[r])
        base += len(rows)
        trans[r] = trans[r] * (1.0 - a)
        taken_n[r] += 1
        drift[r] += sigma * (entry[c] + exit_[c]) * norm[r]
        alive[r] = trans[r] > min_transmittance
        taken.append(c)
        weights.append(weight)
        t0s.append(t0)
    taken = np.concatenate(taken) if taken else np.zeros(0, np.int64)
    weights = np.concatenate(weights) if weights else np.zeros(0)
    t0s = np.concatenate(t0s) if t0s else np.zeros(0)
    rounding = 8.0 * (taken_n + 1) * EPS
    return dict(color=color + trans[:, None] * bg[None, :], alpha=1.0 - trans, depth=depth,
                trans=trans, count=taken_n, gap=w_best - second,
                budget_c=cmax * drift + rounding * max(1.0, cmax, float(np.abs(bg).max())),
                budget_a=drift + rounding, rounding=rounding, clamped=clamped, best=best,
                taken=taken, weights=weights, t0=t0s, entry=entry[taken], cmax=cmax)
