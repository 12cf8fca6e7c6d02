"""A float64 restatement of the K29 distortion contract (include/ffn_hip.h), on the per-crossing
arrays of ``tests/octree_walk_reference.walk``, next to ``octree_grad_reference.gradient``.  Nothing
here walks, and nothing of the package is imported.

The TAKEN crossings of a ray are those of ``octree_volume_reference.composite`` (``leaf >= 0``,
``t_out > t_min``, in order, until ``T <= min_transmittance``).  Per taken leaf k = 1..n:

    t0 = max(t_in, t_min);  L = (t_out - t0) |d|;  m = 0.5 (t0 + t_out) |d|
    sigma = max(stored, 0) (NaN -> 0);  a = 1 - exp(-sigma L);  w = T a;  T <- T (1 - a)
    W_k = sum_{j<k} w_j;  M_k = sum_{j<k} w_j m_j;  I_k = m_k W_k - M_k = sum_{j<k} w_j (m_k - m_j)
    D   = sum_k [ 2 w_k I_k + w_k^2 L_k / 3 ]
    J_k = (M_tot - M_{k+1}) - m_k (W_tot - W_{k+1}) = sum_{j>k} w_j (m_j - m_k)
    G_k = dD/dw_k = 2 (I_k + J_k) + (2/3) w_k L_k
    dD/dsigma_k = L_k [ T_{k+1} G_k - sum_{j>k} w_j G_j ]       0 where stored is negative or NaN

The tail ``sum_{j>k} w_j G_j`` is summed here as it stands, not as ``2 D - prefix``; that the two
agree (``sum_j w_j G_j = 2 D``) is a test of its own.  The gradient of a leaf is the sum over the
rays that take it.

The BUDGETS are derived, not tuned to the kernel, to first order in the sources that
``octree_grad_reference`` counts.  With ``eps = 2^-24`` and, per taken leaf k of a ray,

    e_k     = (entry_k + exit_k) |d|        the f32 rounding of its two plane crossings, as a length
    drift_k = sum_{j<=k} sigma_j e_j         the move of the optical depths in front of and in leaf k
    rho_k   = 12 (k + 1) eps                 f32 rounding steps up to leaf k: the eight of the volume
                                             restatement and m, w m, the sums W and M
    u_k     = drift_k + rho_k                bounds the error of w_j, T_j, T_{k+1} and of W_j = 1 - T_j
                                             for j <= k (|d/dx exp(-x)| <= 1)
    Lam     = the ray's last exit as a length: m <= Lam, and W <= 1
    lam_k   = e_k + 4 eps L_k                the error of L_k
    mu_k    = e_k / 2 + 4 eps Lam            the error of m_k;  muhat_k = max_{j<=k} mu_j

the terms are, step by step:

* ``M_k = sum (T_j - T_{j+1}) m_j``: summed by parts over the ascending m it moves by at most
  ``2 Lam max|dT|`` and by ``sum w_j mu_j <= muhat_k``:  ``nu_k = 2 Lam u_k + muhat_k``.
* ``I_k``: ``iota_k = mu_k W + m dW + dM + 2 eps Lam <= mu_k + Lam u_k + nu_k + 2 eps Lam``; the last
  term is the cancellation in ``m W - M``, one ulp of ``Lam`` per step.
* ``D``: ``sum 2 dw_k I_k`` is summed by parts (I ascends, I <= Lam): ``4 Lam u_n``; then
  ``sum_k [2 w_k iota_k + (2/3) w_k u_k L_k + w_k^2 lam_k / 3]`` and ``6 n eps Lam`` for the f32
  steps of the sum itself:

      b(D) = 4 Lam u_n + 6 n eps Lam + sum_k [ 2 w_k iota_k + (2/3) w_k u_k L_k + w_k^2 lam_k / 3 ]

* ``J_k``: two differences of totals, ``2 nu_n + mu_k + 2 Lam u_n + 3 eps Lam`` (the cancellation in
  ``M_tot - M_{k+1}`` and ``W_tot - W_{k+1}``: one ulp per step).
* ``G_k``: ``gamma_k = 2 (iota_k + dJ_k) + (2/3) (u_k L_k + w_k lam_k) + 4 eps Ghat`` with
  ``Ghat = 2 Lam + (2/3) max L`` a bound of ``G``.
* the tail, which the kernel forms as ``2 D - sum_{j<=k} w_j G_j``: twice ``b(D)``, the prefix's
  ``sum dw_j G_j`` by parts over I (ascending) and J (descending) ``8 Lam u_n + (2/3) u_n max L``,
  ``sum_{j<=k} w_j gamma_j``, and one ulp of ``2 Ghat`` per step for the cancellation:

      tau_k = 2 b(D) + 8 Lam u_n + (2/3) u_n max L + sum_{j<=k} w_j gamma_j + 2 (k + 3) eps Ghat

* ``b(dD/dsigma_k) = lam_k |bracket| + L_k [ u_k G_k + T_{k+1} gamma_k + tau_k + 3 eps Ghat ]``

and per leaf the sum of these over the rays that take it, plus ``m eps sum |term|`` for the f32 sum
of its ``m`` terms in any order."""

import numpy as np

from tests import octree_walk_reference as wref

EPS = 2.0 ** -24
STEPS = 12.0
VARIANTS = ("full", "no_self", "no_tail")


def _taken_steps(w, starts, directions, sigma, t_min, min_transmittance, entry=None, exit_=None):
    """The taken crossings, step by step (step k holds the k-th taken leaf of every ray that has
    one) -> list of dicts of per-row arrays, and the per-ray totals."""
    count = len(w["hit"])
    stored_all = np.asarray(sigma).astype(np.float64).reshape(-1)
    directions = np.asarray(directions, np.float32).reshape(-1, 3).astype(np.float64)
    norm = np.linalg.norm(directions, axis=1)
    with np.errstate(invalid="ignore"):
        qualifies = np.nonzero((w["leaf"] >= 0) & (w["t_out"] > t_min))[0]
    ray = w["ray"][qualifies]
    first_of_ray = np.searchsorted(ray, np.arange(count))
    rank = np.arange(len(ray)) - first_of_ray[ray]
    trans = np.ones(count)
    alive = np.ones(count, bool)
    run_w, run_m, dist = np.zeros(count), np.zeros(count), np.zeros(count)
    drift, reach, taken_n = np.zeros(count), np.zeros(count), np.zeros(count, np.int64)
    longest = np.zeros(count)
    steps = []
    for k in range(int(rank.max()) + 1 if len(rank) else 0):
        rows = np.nonzero(rank == k)[0]
        rows = rows[alive[ray[rows]]]
        if len(rows) == 0:
            break
        r, c = ray[rows], qualifies[rows]
        t0 = np.maximum(w["t_in"][c], t_min)
        t1 = w["t_out"][c]
        length = (t1 - t0) * norm[r]
        mid = 0.5 * (t0 + t1) * norm[r]
        stored = stored_all[w["leaf"][c]]
        sig = np.where(stored > 0, stored, 0.0)
        a = 1.0 - np.exp(-(sig * length))
        weight = trans[r] * a
        inner = mid * run_w[r] - run_m[r]
        dist[r] += 2.0 * weight * inner + weight * weight * length / 3.0
        e = (entry[c] + exit_[c]) * norm[r] if entry is not None else np.zeros(len(r))
        drift[r] += sig * e
        reach[r] = np.maximum(reach[r], np.maximum(np.abs(t0), np.abs(t1)) * norm[r])
        longest[r] = np.maximum(longest[r], length)
        steps.append(dict(r=r, leaf=w["leaf"][c], length=length, mid=mid, stored=stored, a=a,
                          e=e, t_k=trans[r].copy(), weight=weight, w_k=run_w[r].copy(),
                          m_k=run_m[r].copy(), inner=inner, drift=drift[r].copy()))
        run_w[r] += weight
        run_m[r] += weight * mid
        trans[r] = trans[r] * (1.0 - a)
        taken_n[r] += 1
        alive[r] = trans[r] > min_transmittance
    return steps, dict(w_tot=run_w, m_tot=run_m, dist=dist, drift=drift, reach=reach,
                       count=taken_n, longest=longest, trans=trans)


def ray_distortion(w, starts, directions, sigma, t_min=0.0, min_transmittance=0.0):
    """D per ray (R,) f64 alone: what the finite differences of the tests evaluate."""
    return _taken_steps(w, starts, directions, sigma, t_min, min_transmittance)[1]["dist"]


def distortion(w, scale, starts, directions, sigma, t_min=0.0, min_transmittance=0.0,
               variant="full", keep=None):
    """``w``: a ``walk`` result; ``sigma`` (L,) the stored densities; ``keep`` (R,) bool: the rays
    whose gradient is summed (default: all; D is returned for every ray).  ``variant``: "full" is
    the contract; "no_self" drops ``(2/3) w_k L_k`` from ``G_k`` and "no_tail" drops
    ``sum_{j>k} w_j G_j`` -- deliberately WRONG restatements that the tests hold the budget against.

    -> dict: ``dist`` (R,) and ``budget_d`` (R,); ``grad`` (L,) d sigma summed over the kept rays
    and ``budget_g`` (L,); ``taken`` (L,) how many kept rays take the leaf; ``count`` (R,) taken
    leaves per ray; ``wg`` (R,) ``sum_j w_j G_j``; ``reach`` (R,) the last exit as a length."""
    assert variant in VARIANTS
    count = len(w["hit"])
    num_leaves = len(np.asarray(sigma).reshape(-1))
    keep = np.ones(count, bool) if keep is None else np.asarray(keep, bool)
    entry, exit_, _ = wref.budgets(w, scale, starts, directions)
    steps, tot = _taken_steps(w, starts, directions, sigma, t_min, min_transmittance, entry, exit_)
    lam_ray, longest = tot["reach"], tot["longest"]
    u_n = tot["drift"] + STEPS * (tot["count"] + 1) * EPS
    g_hat = 2.0 * lam_ray + (2.0 / 3.0) * longest

    # D's budget, and the per-step errors of m, M and I
    mu_hat = np.zeros(count)
    budget_d = np.zeros(count)
    for k, s in enumerate(steps):
        r = s["r"]
        s["u"] = s["drift"] + STEPS * (k + 1) * EPS
        s["lam"] = s["e"] + 4.0 * EPS * s["length"]
        s["mu"] = 0.5 * s["e"] + 4.0 * EPS * lam_ray[r]
        mu_hat[r] = np.maximum(mu_hat[r], s["mu"])
        nu = 2.0 * lam_ray[r] * s["u"] + mu_hat[r]
        s["iota"] = s["mu"] + lam_ray[r] * s["u"] + nu + 2.0 * EPS * lam_ray[r]
        budget_d[r] += (2.0 * s["weight"] * s["iota"]
                        + (2.0 / 3.0) * s["weight"] * s["u"] * s["length"]
                        + s["weight"] ** 2 * s["lam"] / 3.0)
    budget_d += 4.0 * lam_ray * u_n + 6.0 * tot["count"] * EPS * lam_ray
    nu_n = 2.0 * lam_ray * u_n + mu_hat

    # G, its prefix sums and their budgets
    prefix = np.zeros(count)
    gamma_w = np.zeros(count)
    for s in steps:
        r = s["r"]
        next_w = s["w_k"] + s["weight"]
        next_m = s["m_k"] + s["weight"] * s["mid"]
        outer = (tot["m_tot"][r] - next_m) - s["mid"] * (tot["w_tot"][r] - next_w)
        s["g"] = 2.0 * (s["inner"] + outer)
        if variant != "no_self":
            s["g"] = s["g"] + (2.0 / 3.0) * s["weight"] * s["length"]
        d_outer = 2.0 * nu_n[r] + s["mu"] + 2.0 * lam_ray[r] * u_n[r] + 3.0 * EPS * lam_ray[r]
        s["gamma"] = (2.0 * (s["iota"] + d_outer)
                      + (2.0 / 3.0) * (s["u"] * s["length"] + s["weight"] * s["lam"])
                      + 4.0 * EPS * g_hat[r])
        prefix[r] += s["weight"] * s["g"]
        gamma_w[r] += s["weight"] * s["gamma"]
        s["prefix"] = prefix[r].copy()
        s["gamma_w"] = gamma_w[r].copy()
    total_wg = prefix.copy()

    grad = np.zeros(num_leaves)
    budget_g = np.zeros(num_leaves)
    total = np.zeros(num_leaves)
    taken = np.zeros(num_leaves, np.int64)
    for k, s in enumerate(steps):
        r = s["r"]
        t_next = s["t_k"] * (1.0 - s["a"])
        tail = total_wg[r] - s["prefix"]
        if variant == "no_tail":
            tail = np.zeros(len(r))
        bracket = t_next * s["g"] - tail
        passes = s["stored"] >= 0                              # NaN and negatives: no gradient
        term = np.where(passes, s["length"] * bracket, 0.0)
        tau = (2.0 * budget_d[r] + 8.0 * lam_ray[r] * u_n[r] + (2.0 / 3.0) * u_n[r] * longest[r]
               + s["gamma_w"] + 2.0 * (k + 3) * EPS * g_hat[r])
        b = s["lam"] * np.abs(bracket) + s["length"] * (
            s["u"] * s["g"] + t_next * s["gamma"] + tau + 3.0 * EPS * g_hat[r])
        b = np.where(passes, b, 0.0)
        on = keep[r]
        np.add.at(grad, s["leaf"][on], term[on])
        np.add.at(total, s["leaf"][on], np.abs(term[on]))
        np.add.at(budget_g, s["leaf"][on], b[on])
        np.add.at(taken, s["leaf"][on], 1)
    budget_g += taken * EPS * total
    return dict(dist=tot["dist"], budget_d=budget_d, grad=grad, budget_g=budget_g, taken=taken,
                count=tot["count"], wg=total_wg, trans=tot["trans"], reach=lam_ray)
