"""A float64 restatement of K26 (focus samples from an octree's own weights), written from its
contract (include/ffn_hip.h) on the per-crossing arrays of ``tests/octree_walk_reference.walk``, as
``tests/octree_volume_reference.py`` is for K15.  Nothing here walks.

Of the crossings of a ray those with ``leaf >= 0`` are clipped to ``[near, far]``:

    t0 = max(t_in, near);  t1 = min(t_out, far);  TAKEN iff t1 > t0
    L = (t1 - t0) |d|;  sigma = max(density, 0)  (NaN -> 0)
    a = 1 - exp(-sigma L);  w = T a;  c_next = c + w;  T *= 1 - a

``M`` is ``c`` after the last taken leaf, and the CDF of the ray is

    F(t) = sum_k w_k clip((t - t0_k) / (t1_k - t0_k), 0, 1)

flat in the gaps between taken leaves, linear inside one, continuous and monotone, ``F = M`` from the
last ``t1`` on.  A focus sample for the target ``u`` solves ``F(t) = u M``.  Because F is continuous
the checks need no decision about WHICH leaf a sample belongs to:

(i)   ``t`` lies in ``[t0_k - e_k, t1_k + e_k]`` of some taken leaf k -- never in empty space --
      with ``e_k`` the f32 rounding of that crossing (``octree_walk_reference.budgets``: the entry
      budget at t0, the exit budget at t1; a clipped end moves by no more than the crossing did);
(ii)  ``|F(t) - u M| <= budget``;
(iii) ``|mass_out - M| <= budget_a``.

The BUDGET of (ii) is derived here, not tuned to the kernel.  With ``x_j = sigma_j L_j`` the optical
depth of taken leaf j and ``dx_j = sigma_j (entry_j + exit_j) |d|`` its error from the two crossings:

1. ``budget_a``, the alpha budget of ``octree_volume_reference`` over the taken leaves (those
   clipped at ``far`` included, none beyond it), ``sum_j dx_j + 8 (n + 1) 2^-24``, with ONE
   refinement that only ever lowers it: the volume reference bounds ``|d/dx exp(-x)|`` by 1, here it
   is bounded by its largest value on the interval, ``exp(-max(x_j - dx_j, 0))`` (mean value
   theorem), so ``drift = sum_j dx_j exp(-max(x_j - dx_j, 0))``.  Without it an opaque leaf (sigma
   1e30) has a budget of 1e24 and every check on its rays is void; with it such a leaf costs nothing,
   as it should: no crossing error makes it less than opaque.
   The kernel places the target where ITS running sum c~ passes u M~, so the error is
   ``E_k - u E_n`` with ``E_k`` the error of the sum at the sample's leaf k and ``E_n`` that of M.
   Both sums grow with every x_j (``d c_k / d x_j = T_{k+1}`` for j <= k, ``d M / d x_j = T_{n+1}``,
   both in [0, 1]), so the coefficient of dx_j in the difference is at most 1 in magnitude: the
   drift counts ONCE.  The rounding part ``8 (n + 1) 2^-24`` (eight f32 roundings per leaf step, see
   the volume reference) has no such sign and counts once for c~ and once for u M~: it is added a
   second time.
2. ``steepest (e_ray + 4 ulp(t_max))``: a ramp whose ends are off by the ray's largest crossing
   budget ``e_ray``, evaluated at a t that carries the roundings of ``t1 - t0``, the product with f,
   the sum with t0 and the chord ends themselves (four, each at most an ulp of the largest |t| on
   the chord), moves F by at most its slope times that.  Inside leaf k the slope is
   ``w_k / (t1_k - t0_k) <= sigma_k |d|`` (``1 - exp(-x) <= x``, T <= 1); ``steepest`` is the largest
   over the ray's taken leaves of ``min(sigma_k |d|, w_k / (chord_k - entry_k - exit_k))``, the
   second form being the slope itself on the shortest chord the roundings allow (what keeps the
   term finite on an opaque leaf; infinite, and the check void, only on a chord shorter than its
   own rounding).
3. ``6 * 2^-24``: the roundings of ``y = u M``, ``y - c``, the quotient by w, and once more each for
   the three operations of item 2 where they act on f rather than t -- relative roundings of values
   that map to at most F <= 1.

A ray with ``|M - min_mass| <= budget_a`` is UNDECIDED (the kernel may or may not take the
fall-back); the tests choose scenes without any and assert it.

``focus32`` is a plain numpy-f32 restatement of the kernel's operation list on the same crossings
(rounded to f32 once: a crossing of the kernel is a rounded quotient too): it shows that the budgets
can be met before a GPU sees them, and gives known answers where f32 is exact."""

import numpy as np

from tests import octree_walk_reference as wref

EPS = 2.0 ** -24


def _ulp(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def cdf(w, scale, starts, directions, near, far, sigma):
    """``w``: a ``walk`` result over ``starts`` (relative to the cube's centre) / ``directions``;
    ``near``, ``far`` (R,) f32; ``sigma`` (L,) the density of every leaf as the kernel reads it.
    -> dict: per ray (R,) ``mass``, ``count``, ``budget_a``, ``rounding``, ``slope`` (item 2 of the
    budget), ``budget`` (items 1 + 2 + 3); per taken leaf (K,) ``ray``, ``t0``, ``t1``, ``weight``,
    ``before`` (c ahead of it), ``e0``, ``e1`` (the crossing budgets at its two ends), sorted by ray
    and t; ``first`` (R + 1,) offsets of the rays in those arrays."""
    count = len(w["hit"])
    directions = np.asarray(directions, np.float32).reshape(-1, 3).astype(np.float64)
    near = np.asarray(near, np.float32).astype(np.float64)
    far = np.asarray(far, np.float32).astype(np.float64)
    sigma = np.asarray(sigma).astype(np.float64)
    sigma = np.where(sigma > 0, sigma, 0.0)                      # NaN and negatives: 0
    norm = np.linalg.norm(directions, axis=1)
    entry, exit_, per_ray = wref.budgets(w, scale, starts, directions)

    ray = w["ray"]
    with np.errstate(invalid="ignore"):
        t0 = np.maximum(w["t_in"], near[ray])
        t1 = np.minimum(w["t_out"], far[ray])
        take = np.nonzero((w["leaf"] >= 0) & (t1 > t0) & (near[ray] < far[ray]))[0]
    ray, t0, t1 = ray[take], t0[take], t1[take]
    s = sigma[w["leaf"][take]]
    e0, e1 = entry[take], exit_[take]
    first = np.searchsorted(ray, np.arange(count + 1))
    rank = np.arange(len(ray)) - first[ray]

    trans = np.ones(count)
    mass = np.zeros(count)
    drift = np.zeros(count)
    taken_n = np.zeros(count, np.int64)
    steepest = np.zeros(count)
    t_max = np.zeros(count)
    weight = np.zeros(len(ray))
    before = np.zeros(len(ray))
    for k in range(int(rank.max()) + 1 if len(rank) else 0):
        rows = np.nonzero(rank == k)[0]
        r = ray[rows]
        a = 1.0 - np.exp(-(s[rows] * ((t1[rows] - t0[rows]) * norm[r])))
        weight[rows] = trans[r] * a
        before[rows] = mass[r]
        mass[r] = mass[r] + weight[rows]
        trans[r] = trans[r] * (1.0 - a)
        x = s[rows] * ((t1[rows] - t0[rows]) * norm[r])
        dx = s[rows] * (e0[rows] + e1[rows]) * norm[r]
        drift[r] += dx * np.exp(-np.maximum(x - dx, 0.0))
        taken_n[r] += 1
        with np.errstate(divide="ignore", invalid="ignore"):
            chord = (t1[rows] - t0[rows]) - (e0[rows] + e1[rows])
            ramp = np.where(chord > 0, weight[rows] / chord, np.inf)
        steepest[r] = np.maximum(steepest[r], np.minimum(s[rows] * norm[r], ramp))
        t_max[r] = np.maximum(t_max[r], np.maximum(np.abs(t0[rows]), np.abs(t1[rows])))
    rounding = 8.0 * (taken_n + 1) * EPS
    budget_a = drift + rounding
    slope = steepest * (per_ray + 4.0 * _ulp(t_max))
    return dict(mass=mass, count=taken_n, budget_a=budget_a, rounding=rounding, slope=slope,
                budget=budget_a + rounding + slope + 6.0 * EPS, ray=ray, t0=t0, t1=t1,
                weight=weight, before=before, e0=e0, e1=e1, first=first)


def evaluate(c, r, t):
    """F(t) of ray ``r`` at the values ``t`` (any shape), float64."""
    lo, hi = c["first"][r], c["first"][r + 1]
    t = np.asarray(t, np.float64)
    t0, t1, wk = c["t0"][lo:hi], c["t1"][lo:hi], c["weight"][lo:hi]
    part = np.clip((t[..., None] - t0) / (t1 - t0), 0.0, 1.0)
    return (part * wk).sum(-1)


def inside_taken(c, r, t):
    """Check (i): per value of ``t`` whether it lies in some taken leaf of ray ``r``, the leaf
    widened by its crossing budgets."""
    lo, hi = c["first"][r], c["first"][r + 1]
    t = np.asarray(t, np.float64)[..., None]
    return ((t >= c["t0"][lo:hi] - c["e0"][lo:hi]) & (t <= c["t1"][lo:hi] + c["e1"][lo:hi])).any(-1)


def undecided(c, min_mass):
    return np.abs(c["mass"] - np.float64(np.float32(min_mass))) <= c["budget_a"]


def fallback32(near, far, u):
    """The uniform fall-back, numpy f32 operation by operation: (R,), (R,), (R,n) -> (R,n)."""
    near = np.asarray(near, np.float32)[:, None]
    far = np.asarray(far, np.float32)[:, None]
    u = np.asarray(u, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        ordered = near < far
        return np.where(ordered, near + u * (far - near), near + np.zeros_like(u)).astype(np.float32)


def check(c, near, far, u, min_mass, t_focus, mass_out, what=""):
    """Asserts the focus-only rows ``t_focus`` (R, n_focus) f32 and ``mass_out`` (R,) f32 of a K26
    call against the restatement ``c``: no undecided ray; the mass; rows ascending and inside
    ``[near, far]``; the fall-back rows bit for bit; (i) and (ii) for the rays with mass.  NaN targets
    are left out of (ii).  -> the worst error / budget of (ii)."""
    near = np.asarray(near, np.float32)
    far = np.asarray(far, np.float32)
    u = np.asarray(u, np.float32)
    count = len(near)
    assert t_focus.shape == u.shape and t_focus.dtype == np.float32
    assert not undecided(c, min_mass).any(), "an undecided ray: choose another scene"
    err_m = np.abs(mass_out.astype(np.float64) - c["mass"])
    assert (err_m <= c["budget_a"]).all(), (what, err_m.max())
    with_mass = c["mass"] >= np.float64(np.float32(min_mass))
    with np.errstate(invalid="ignore"):
        ordered = near < far
    assert not (with_mass & ~ordered).any()
    # the fall-back, bit for bit
    flat = fallback32(near, far, u)
    rows = ~with_mass
    assert (t_focus[rows].view(np.uint32) == flat[rows].view(np.uint32)).all(), what
    # ascending, inside [near, far]
    clean = ~np.isnan(u).any(1) & ordered
    assert (np.diff(t_focus[clean], axis=1) >= 0).all(), what
    assert (t_focus[clean] >= near[clean, None]).all() and (t_focus[clean] <= far[clean, None]).all()
    worst = 0.0
    for r in np.nonzero(with_mass)[0]:
        t = t_focus[r].astype(np.float64)
        assert inside_taken(c, r, t).all(), (what, r, "a sample in empty space")
        assert (np.diff(t) >= 0).all() and t[0] >= near[r] and t[-1] <= far[r], (what, r)
        known = ~np.isnan(u[r])
        err = np.abs(evaluate(c, r, t) - u[r].astype(np.float64) * c["mass"][r])[known]
        worst = max(worst, float((err / c["budget"][r]).max()) if known.any() else 0.0)
        assert (err <= c["budget"][r]).all(), (what, r, err.max(), c["budget"][r])
    return worst


def focus32(w, directions, near, far, sigma, u, min_mass, uniform=None):
    """The kernel's operation list in numpy f32, one ray at a time, on the crossings of ``w`` rounded
    to f32.  ``u`` (R, n_focus) f32, ``uniform`` (R, n_uniform) f32 or None.
    -> t (R, n_uniform + n_focus) f32, mass (R,) f32."""
    f32 = np.float32
    directions = np.asarray(directions, f32).reshape(-1, 3)
    near = np.asarray(near, f32)
    far = np.asarray(far, f32)
    sigma = np.asarray(sigma, f32)
    u = np.asarray(u, f32)
    min_mass = f32(min_mass)
    count, n_focus = u.shape
    t_in, t_out = w["t_in"].astype(f32), w["t_out"].astype(f32)
    focus = np.zeros((count, n_focus), f32)
    masses = np.zeros(count, f32)
    zero, one = f32(0), f32(1)
    with np.errstate(all="ignore"):
        for r in range(count):
            lo, hi = int(w["offsets"][r]), int(w["offsets"][r + 1])
            dx, dy, dz = directions[r]
            norm = np.sqrt((dx * dx + dy * dy) + dz * dz)
            ordered = bool(near[r] < far[r])
            mass, t_last, last, j = zero, near[r], f32(-np.inf), 0
            use_tree = False
            for phase in range(2):
                if phase == 1:
                    use_tree = bool(mass > zero) and bool(mass >= min_mass)
                    if not use_tree:
                        break
                trans, c = one, zero
                y = u[r, 0] * mass if phase == 1 else zero
                for k in range(lo, hi if (w["hit"][r] and ordered) else lo):
                    if w["leaf"][k] >= 0:
                        t0 = max(t_in[k], near[r])
                        t1 = min(t_out[k], far[r])
                        if t1 > t0:
                            ls = sigma[w["leaf"][k]]
                            length = (t1 - t0) * norm
                            s = ls if ls > zero else zero
                            a = one - np.exp(-(s * length))
                            wk = trans * a
                            c_next = c + wk
                            if wk > zero:
                                t_last = t1
                                if phase == 1:
                                    while j < n_focus and y < c_next:
                                        fr = (y - c) / wk
                                        v = min(max(t0 + fr * (t1 - t0), t0), t1)
                                        v = max(v, last)
                                        focus[r, j] = v
                                        last = v
                                        j += 1
                                        y = u[r, j] * mass if j < n_focus else zero
                            c = c_next
                            trans = trans * (one - a)
                            if trans == zero or (phase == 1 and j >= n_focus):
                                break
                    if not t_out[k] < far[r]:
                        break
                if phase == 0:
                    mass = c
            masses[r] = mass
            if use_tree:
                focus[r, j:] = max(t_last, last)
            else:
                focus[r] = fallback32(near[r:r + 1], far[r:r + 1], u[r:r + 1])[0]
    if uniform is None:
        return focus, masses
    merged = np.sort(np.concatenate([np.asarray(uniform, f32), focus], axis=1), axis=1)
    return merged, masses
