"""A float64 restatement of the K17 gradient contract (include/ffn_hip.h), on the per-crossing
arrays of ``tests/octree_walk_reference.walk``, next to ``octree_volume_reference.composite``.
Nothing here walks.

The TAKEN crossings of a ray are those of ``composite`` (``leaf >= 0``, ``t_out > t_min``, in order,
until ``T <= min_transmittance``).  With ``x_k = sigma_k L_k``, ``a_k = 1 - exp(-x_k)``, ``T_k`` the
transmittance in front of taken leaf k, ``w_k = T_k a_k``, ``C = sum w_k c_k + T_{n+1} bg`` and the
upstream gradients ``g_C`` (3,), ``g_A``:

    d c_k     = w_k g_C
    d sigma_k = L_k [ g_C . (T_{k+1} c_k - S_k) + g_A T_{n+1} ],   S_k = C - sum_{j<=k} w_j c_j

``d sigma_k`` is 0 where the stored density is negative or NaN; the gradient of a leaf is the sum
over the rays that take it.

The BUDGET of a leaf is derived, not tuned to the kernel, to first order in the sources that
``octree_volume_reference`` counts.  Per taken leaf k of a ray, with ``M = max(1, cmax, |bg|)``,
``e_k = (entry_k + exit_k) |d|`` the f32 rounding of its two plane crossings as a length,
``drift_k = sum_{j<=k} sigma_j e_j`` (every ``w``, ``T`` and prefix colour moves by at most the
change of the optical depths in front of it, ``|d/dx exp(-x)| <= 1``), ``r_k = 8 (k + 1) 2^-24`` the
rounding steps up to leaf k (eight per leaf as in the volume restatement; the cancellation in
``C - prefix`` is one ulp of M per step and counted among them) and ``n`` the ray's last leaf:

    b(d c_k)     = |g_C|_max (drift_k + r_k)
    b(d sigma_k) = (e_k + 4 2^-24 L_k) B
                   + L_k [ |g_C|_1 ( cmax (drift_k + r_k)                       T_{k+1} c_k
                                     + cmax drift_n + r_n M                     C
                                     + cmax drift_k + r_k M )                   the prefix
                           + |g_A| (drift_n + r_n) ]                            T_{n+1}
    B            = 2 M |g_C|_1 + |g_A|          (a bound of the bracket)

and per leaf the sum of these over the rays that take it, plus ``m 2^-24 sum |term|`` for the f32
sum of its ``m`` terms in any order."""

import numpy as np

from tests import octree_volume_reference as vref
from tests import octree_walk_reference as wref

EPS = 2.0 ** -24


def gradient(w, scale, starts, directions, leaf_data, d_color, d_alpha, t_min=0.0,
             background=(0.0, 0.0, 0.0), min_transmittance=0.0):
    """``w``: a ``walk`` result; leaf_data (L, C >= 4); d_color (R,3), d_alpha (R,).  -> dict:
    ``grad`` (L,4) f64, ``budget`` (L,4), ``taken`` (L,) how many rays take the leaf."""
    count = len(w["hit"])
    data = np.asarray(leaf_data).astype(np.float64)
    num_leaves = len(data)
    bg = np.asarray(background, np.float32).astype(np.float64)
    g_c = np.asarray(d_color).astype(np.float64).reshape(count, 3)
    g_a = np.asarray(d_alpha).astype(np.float64).reshape(count)
    directions = np.asarray(directions, np.float32).reshape(-1, 3).astype(np.float64)
    norm = np.linalg.norm(directions, axis=1)
    entry, exit_, _ = wref.budgets(w, scale, starts, directions)
    v = vref.composite(w, scale, starts, directions, leaf_data, t_min, background,
                       min_transmittance)
    final_c, final_t = v["color"], v["trans"]
    cmax = float(np.abs(data[:, :3]).max())
    big = max(1.0, cmax, float(np.abs(bg).max()))

    with np.errstate(invalid="ignore"):
        qualifies = np.nonzero((w["leaf"] >= 0) & (w["t_out"] > t_min))[0]
    ray = w["ray"][qualifies]
    first_of_ray = np.searchsorted(ray, np.arange(count))
    rank = np.arange(len(ray)) - first_of_ray[ray]

    # the whole ray's drift and rounding first (n is known only at the end of a ray)
    drift_n = np.zeros(count)
    trans = np.ones(count)
    alive = np.ones(count, bool)
    steps = []
    for k in range(int(rank.max()) + 1 if len(rank) else 0):
        rows = np.nonzero(rank == k)[0]
        rows = rows[alive[ray[rows]]]
        if len(rows) == 0:
            break
        r, c = ray[rows], qualifies[rows]
        t0 = np.maximum(w["t_in"][c], t_min)
        length = (w["t_out"][c] - t0) * norm[r]
        stored = data[w["leaf"][c], 3]
        sigma = np.where(stored > 0, stored, 0.0)
        a = 1.0 - np.exp(-(sigma * length))
        e = (entry[c] + exit_[c]) * norm[r]
        drift_n[r] += sigma * e
        steps.append((r, c, length, stored, sigma, a, e, trans[r].copy(), drift_n[r].copy()))
        trans[r] = trans[r] * (1.0 - a)
        alive[r] = trans[r] > min_transmittance
    r_n = 8.0 * (v["count"] + 1) * EPS

    grad = np.zeros((num_leaves, 4))
    budget = np.zeros((num_leaves, 4))
    total = np.zeros((num_leaves, 4))
    taken = np.zeros(num_leaves, np.int64)
    prefix = np.zeros((count, 3))
    for k, (r, c, length, stored, sigma, a, e, t_k, drift_k) in enumerate(steps):
        leaf = w["leaf"][c]
        rgb = data[leaf, :3]
        weight = t_k * a
        prefix[r] += weight[:, None] * rgb
        t_next = t_k * (1.0 - a)
        behind = final_c[r] - prefix[r]
        bracket = (g_c[r] * (t_next[:, None] * rgb - behind)).sum(1) + g_a[r] * final_t[r]
        passes = stored >= 0                                  # NaN and negatives: no gradient
        term = np.concatenate([weight[:, None] * g_c[r],
                               np.where(passes, length * bracket, 0.0)[:, None]], 1)
        r_k = 8.0 * (k + 1) * EPS
        g1, gmax, ga = np.abs(g_c[r]).sum(1), np.abs(g_c[r]).max(1), np.abs(g_a[r])
        b_color = gmax * (drift_k + r_k)
        bound = 2.0 * big * g1 + ga
        b_sigma = (e + 4.0 * EPS * length) * bound + length * (
            g1 * (cmax * (drift_k + r_k) + cmax * drift_n[r] + r_n[r] * big
                  + cmax * drift_k + r_k * big) + ga * (drift_n[r] + r_n[r]))
        b_sigma = np.where(passes, b_sigma, 0.0)
        np.add.at(grad, leaf, term)
        np.add.at(total, leaf, np.abs(term))
        np.add.at(budget, leaf, np.concatenate([np.repeat(b_color[:, None], 3, 1),
                                                b_sigma[:, None]], 1))
        np.add.at(taken, leaf, 1)
    budget += taken[:, None] * EPS * total
    return dict(grad=grad, budget=budget, taken=taken, composite=v)
