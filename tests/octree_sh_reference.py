"""A float64 restatement of the K18a SH volume render, written from its contract
(include/ffn_hip.h).  The walk and the compositing are those of ``tests/octree_volume_reference.py``
(which runs on the crossings of ``tests/octree_walk_reference.walk``); only the colour of a leaf is
replaced: for ray direction ``d`` and ``u = d / |d|`` (not negated),

    colour_c = sigmoid(sum_b k[c B + b] Y_b(u)),      B = (degree + 1)^2

with ``leaf_data`` rows ``[k_r0 .. k_r(B-1), k_g0 .., k_b0 .., sigma]`` and ``Y`` written out below
from the closed forms, not imported from the package.

The BUDGET of a ray is derived, not tuned to the kernel.  ``budget_a`` is K15's.  ``budget_c`` is
K15's with ``cmax = 1`` (a sigmoid is at most 1) plus the colour's own rounding, weighted by the
leaf's weight ``w_k`` (``sum w <= 1``).  With ``eps = 2^-24``, per taken leaf and channel:

* the normalisation: ``|d|`` in f32 is three products, two sums and a square root, within 2.5 eps
  relative; its reciprocal and the product with a component add one rounding each: a component of
  ``u`` is within 5 eps.  A band-1 term is ``0.4886 u_i`` (its constant and its product round once
  each): within ``0.4886 (5 + 2) eps <= 3.5 eps``.  A band-2 term is a quadratic form whose gradient
  over the unit sphere is at most 1.6 (``1.0925 sqrt 2``, ``0.3154 sqrt 24``, ``0.5463 * 2 sqrt 2``),
  evaluated with at most six roundings of values of at most 2 times a constant of at most 1.0925,
  halved by the constants of the longest form: within ``(5 * 1.6 + 6) eps = 14 eps``.  Band 0 is a
  constant: 0.3 eps.  Together ``sum_b |k_cb| E_b eps`` with ``E = [0.3, 3.5 x3, 14 x5]``.
* the dot product: a chain of B operations, each rounding a partial sum of at most
  ``S = sum_b |k_cb| |Y_b|``: ``B S eps``.
* the sigmoid's slope is at most 1/4, so the logit's error enters the colour with that factor;
  ``1 / (1 + expf(-z))`` itself is within 6 eps: ``expf`` within 2 ulp = 4 eps relative, the sum and
  the quotient one rounding each, and the relative error of ``1 / (1 + e)`` is at most that of
  ``e``.

    delta_k = max_c [ (sum_b |k_cb| E_b + B S_c) / 4 + 6 ] eps
    budget_c = budget_a + rounding * (max(1, |bg|) - 1) + sum_k w_k delta_k
"""

import numpy as np

from tests import octree_volume_reference as vref

EPS = 2.0 ** -24
BAND_ERROR = np.array([0.3, 3.5, 3.5, 3.5, 14.0, 14.0, 14.0, 14.0, 14.0])


def basis(directions, degree):
    """(R,3) directions of any length -> (R, B) float64, from the closed forms."""
    d = np.asarray(directions, np.float32).reshape(-1, 3).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        u = d / np.linalg.norm(d, axis=1, keepdims=True)
    x, y, z = u[:, 0], u[:, 1], u[:, 2]
    terms = [np.full(len(u), 0.28209479177387814), -0.4886025119029199 * y,
             0.4886025119029199 * z, -0.4886025119029199 * x]
    if degree == 2:
        terms += [1.0925484305920792 * x * y, -1.0925484305920792 * y * z,
                  0.31539156525252005 * (2 * z * z - x * x - y * y),
                  -1.0925484305920792 * x * z, 0.5462742152960396 * (x * x - y * y)]
    return np.stack(terms, 1)


def leaf_colors(leaf_data, degree, y):
    """Per (row of leaf_data, row of y): colour (K,3) and the rounding term delta (K,)."""
    bases = (degree + 1) ** 2
    k = np.asarray(leaf_data, np.float64)[:, :3 * bases].reshape(-1, 3, bases)
    z = (k * y[:, None, :]).sum(2)
    size = (np.abs(k) * np.abs(y[:, None, :])).sum(2)
    drift = (np.abs(k) * BAND_ERROR[None, None, :bases]).sum(2)
    delta = ((drift + bases * size) / 4.0 + 6.0).max(1) * EPS
    return 1.0 / (1.0 + np.exp(-z)), delta


def composite(w, scale, starts, directions, leaf_data, degree, t_min=0.0,
              background=(0.0, 0.0, 0.0), min_transmittance=0.0):
    """``leaf_data`` (L, 3B+1) in the file's order.  -> the dict of
    ``octree_volume_reference.composite`` for the densities of the last column, with ``color`` and
    ``budget_c`` those of the SH colour."""
    leaf_data = np.asarray(leaf_data)
    bases = (degree + 1) ** 2
    assert leaf_data.shape[1] == 3 * bases + 1
    plain = np.zeros((len(leaf_data), 4), np.float64)
    plain[:, 3] = leaf_data[:, -1]
    v = vref.composite(w, scale, starts, directions, plain, t_min, background, min_transmittance)
    bg = np.asarray(background, np.float32).astype(np.float64)
    count = len(w["hit"])
    color = np.zeros((count, 3))
    own = np.zeros(count)
    if len(v["taken"]):
        ray, leaf = w["ray"][v["taken"]], w["leaf"][v["taken"]]
        rgb, delta = leaf_colors(leaf_data[leaf], degree, basis(directions, degree)[ray])
        np.add.at(color, ray, v["weights"][:, None] * rgb)
        np.add.at(own, ray, v["weights"] * delta)
    v["color"] = color + v["trans"][:, None] * bg[None, :]
    v["budget_c"] = (v["budget_a"] + v["rounding"] * (max(1.0, float(np.abs(bg).max())) - 1.0)
                     + own)
    v["own"] = own
    return v
