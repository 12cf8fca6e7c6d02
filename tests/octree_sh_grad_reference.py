"""A float64 restatement of the K19 gradient contract (include/ffn_hip.h), on the per-crossing
arrays of ``tests/octree_walk_reference.walk``, next to ``octree_grad_reference.gradient`` (K17) and
``octree_sh_reference.composite`` (K18a).  Nothing here walks, and nothing is imported from the
package.

The TAKEN crossings of a ray are those of the volume restatement.  With ``x_k = sigma_k L_k``,
``a_k = 1 - exp(-x_k)``, ``T_k`` the transmittance in front of taken leaf k, ``w_k = T_k a_k``, the
leaf's colour ``c_k = sigmoid(z_k)``, ``z_kc = sum_b k_cb Y_b(u)`` at the ray's unit direction ``u``,
``C = sum w_k c_k + T_{n+1} bg`` and the upstream gradients ``g_C`` (3,), ``g_A``:

    d k_cb    = e_kc Y_b(u),    e_kc = w_k g_c c_kc (1 - c_kc)
    d sigma_k = L_k [ g_C . (T_{k+1} c_k - S_k) + g_A T_{n+1} ],   S_k = C - sum_{j<=k} w_j c_j

``d sigma_k`` is 0 where the stored density is negative or NaN; the gradient of a leaf is the sum
over the rays that take it.  ``grad`` is (L, 3B+1) in the FILE order ``[k_r.., k_g.., k_b.., sigma]``.

The BUDGET of a leaf and channel is derived, not tuned to the kernel.  It is K17's
(``octree_grad_reference``) with ``cmax = 1`` (a sigmoid is at most 1), ``M = max(1, |bg|)``, the
same ``e_k``, ``drift_k``, ``r_k = 8 (k + 1) eps`` and ``n``, ``eps = 2^-24``, plus what the colour
adds.  ``delta_k`` is the rounding of leaf k's colour in K18a (``octree_sh_reference.leaf_colors``:
basis, dot product, sigmoid), ``own_k = sum_{j<=k} w_j delta_j``, ``E_b`` the basis error per band
(``octree_sh_reference.BAND_ERROR``, in units of eps), ``s_kc = c_kc (1 - c_kc) <= 1/4``.

Density.  K17's ``b(d sigma_k)`` has the colour exact.  Here ``c_k`` is off by ``delta_k`` where it
stands in the bracket: ``T_{k+1} c_k`` moves by ``T_{k+1} delta_k``, ``C`` by ``own_n`` and the
prefix by ``own_k``:

    b(d sigma_k) = K17's with cmax = 1  +  L_k |g_C|_1 (T_{k+1} delta_k + own_n + own_k)

Coefficients.  ``e_kc`` is the product of ``w_k g_c`` -- K17's ``d c_k``, budget ``|g_c| (drift_k +
r_k)`` -- and the slope ``s_kc``.  The slope is computed from the rounded colour: ``|d/dc c (1 - c)|
= |1 - 2 c| <= 1``, so it is off by at most ``delta_k``, and ``s (1 - s)`` and the two products add
three roundings, taken as ``4 eps`` relative:

    b(e_kc)   = |g_c| ( s_kc (drift_k + r_k) + w_k delta_k ) + 4 eps |e_kc|
    b(d k_cb) = |Y_b| b(e_kc) + |e_kc| (E_b + |Y_b|) eps

the last term being the basis value's own error and the rounding of the product with it.

Per leaf and channel the budget is the sum of these over the rays that take the leaf, plus
``m 2^-24 sum |term|`` for the f32 sum of its ``m`` terms in any order.

``variant`` restates the contract WRONGLY, for the tests that show the comparison can fail:
``"flipped"`` takes the basis of ``-u`` (odd bands change sign), ``"slope"`` replaces ``c (1 - c)``
by ``c``, ``"short"`` drops the last entry (in ray order) of the longest list."""

import numpy as np

from tests import octree_sh_reference as sref
from tests import octree_volume_reference as vref
from tests import octree_walk_reference as wref

EPS = 2.0 ** -24
VARIANTS = (None, "flipped", "slope", "short")


def gradient(w, scale, starts, directions, leaf_data, degree, d_color, d_alpha, t_min=0.0,
             background=(0.0, 0.0, 0.0), min_transmittance=0.0, variant=None):
    """``w``: a ``walk`` result; leaf_data (L, 3B+1) in the file's order; d_color (R,3), d_alpha
    (R,).  -> dict: ``grad`` (L, 3B+1) f64, ``budget`` (L, 3B+1), ``taken`` (L,) how many rays take
    the leaf, ``composite`` the SH restatement's render."""
    assert variant in VARIANTS
    bases = (degree + 1) ** 2
    count = len(w["hit"])
    data = np.asarray(leaf_data).astype(np.float64)
    assert data.shape[1] == 3 * bases + 1
    num_leaves = len(data)
    bg = np.asarray(background, np.float32).astype(np.float64)
    g_c = np.asarray(d_color).astype(np.float64).reshape(count, 3)
    g_a = np.asarray(d_alpha).astype(np.float64).reshape(count)
    directions = np.asarray(directions, np.float32).reshape(-1, 3).astype(np.float64)
    norm = np.linalg.norm(directions, axis=1)
    entry, exit_, _ = wref.budgets(w, scale, starts, directions)
    v = sref.composite(w, scale, starts, directions, leaf_data, degree, t_min, background,
                       min_transmittance)
    final_c, final_t, own_n = v["color"], v["trans"], v["own"]
    big = max(1.0, float(np.abs(bg).max()))
    y_true = sref.basis(directions, degree)
    y_used = sref.basis(-directions, degree) if variant == "flipped" else y_true
    band = sref.BAND_ERROR[:bases]

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
        stored = data[w["leaf"][c], -1]
        sigma = np.where(stored > 0, stored, 0.0)
        a = 1.0 - np.exp(-(sigma * length))
        e = (entry[c] + exit_[c]) * norm[r]
        drift_n[r] += sigma * e
        steps.append((r, c, length, stored, a, e, trans[r].copy(), drift_n[r].copy()))
        trans[r] = trans[r] * (1.0 - a)
        alive[r] = trans[r] > min_transmittance
    r_n = 8.0 * (v["count"] + 1) * EPS

    width = 3 * bases + 1
    terms, budgets, leaves_of, rays_of = [], [], [], []
    prefix = np.zeros((count, 3))
    own_k = np.zeros(count)
    for k, (r, c, length, stored, a, e, t_k, drift_k) in enumerate(steps):
        leaf = w["leaf"][c]
        rgb, delta = sref.leaf_colors(data[leaf], degree, y_true[r])
        weight = t_k * a
        prefix[r] += weight[:, None] * rgb
        own_k[r] += weight * delta
        t_next = t_k * (1.0 - a)
        behind = final_c[r] - prefix[r]
        bracket = (g_c[r] * (t_next[:, None] * rgb - behind)).sum(1) + g_a[r] * final_t[r]
        passes = stored >= 0                                  # NaN and negatives: no gradient
        slope = rgb if variant == "slope" else rgb * (1.0 - rgb)
        e_kc = weight[:, None] * g_c[r] * slope                               # (m, 3)
        term = np.concatenate([(e_kc[:, :, None] * y_used[r][:, None, :]).reshape(len(r), -1),
                               np.where(passes, length * bracket, 0.0)[:, None]], 1)
        r_k = 8.0 * (k + 1) * EPS
        g1, ga = np.abs(g_c[r]).sum(1), np.abs(g_a[r])
        true_slope = rgb * (1.0 - rgb)
        true_e = np.abs(weight[:, None] * g_c[r] * true_slope)
        b_e = np.abs(g_c[r]) * (true_slope * (drift_k + r_k)[:, None]
                                + (weight * delta)[:, None]) + 4.0 * EPS * true_e
        y_abs = np.abs(y_true[r])
        b_k = (y_abs[:, None, :] * b_e[:, :, None]
               + true_e[:, :, None] * (band[None, None, :] + y_abs[:, None, :]) * EPS)
        bound = 2.0 * big * g1 + ga
        b_sigma = (e + 4.0 * EPS * length) * bound + length * (
            g1 * ((drift_k + r_k) + drift_n[r] + r_n[r] * big + drift_k + r_k * big)
            + ga * (drift_n[r] + r_n[r])
            + g1 * (t_next * delta + own_n[r] + own_k[r]))
        b_sigma = np.where(passes, b_sigma, 0.0)
        terms.append(term)
        budgets.append(np.concatenate([b_k.reshape(len(r), -1), b_sigma[:, None]], 1))
        leaves_of.append(leaf)
        rays_of.append(r)
    grad = np.zeros((num_leaves, width))
    budget = np.zeros((num_leaves, width))
    total = np.zeros((num_leaves, width))
    taken = np.zeros(num_leaves, np.int64)
    dropped = None
    if terms:
        terms, budgets = np.concatenate(terms), np.concatenate(budgets)
        leaves_of, rays_of = np.concatenate(leaves_of), np.concatenate(rays_of)
        np.add.at(taken, leaves_of, 1)
        keep = np.ones(len(terms), bool)
        if variant == "short":
            longest = int(np.argmax(taken))
            members = np.nonzero(leaves_of == longest)[0]
            keep[members[np.argmax(rays_of[members])]] = False
            dropped = longest
        np.add.at(grad, leaves_of[keep], terms[keep])
        np.add.at(total, leaves_of, np.abs(terms))
        np.add.at(budget, leaves_of, budgets)
    budget += taken[:, None] * EPS * total
    return dict(grad=grad, budget=budget, taken=taken, composite=v, dropped=dropped)

