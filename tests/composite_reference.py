"""Float64 reference of the compositing and loss kernels (csrc/composite.hip, csrc/composite_terms.h)
with a first-order error budget for every output element.

What is checked, on the kernels' own (exact f32) inputs:

* K5   ``ffn_composite_fwd``     colour, alpha, depth            (ray_caster.py:66-93)
* K5w  ``ffn_blend_weights``     weights                         (utils.py:72-97)
* K5w' ``ffn_blend_weights_bwd`` d_sigma, d_t                    (autograd of utils.py:72-97)
* K5b  ``ffn_composite_bwd``     d_logits                        (autograd of ray_caster.py:66-93)
* K6   ``ffn_mse_loss``          loss sums, d_colour, d_alpha    (image_dataset.py:224-262)
* K5t  ``ffn_composite_train``   d_logits, per-workgroup partials
* ``ffn_loss_from_partials`` / ``ffn_loss_value``: sums and the scalar loss

Every element is held to ``|got - ref| <= kappa * 2^-24 * budget``.  The budget is carried by
:class:`V`, a float64 value together with ``b``, a first-order bound on the error an f32 evaluation
of the same expression can have, in units of ``u = 2^-24``:

* a rounded result ``r`` adds ``|r|`` (plus ``2^-126``: a rounding in the denormal range is
  ``2^-150`` absolute);
* ``a + b`` carries ``b_a + b_b``; ``a b`` carries ``|a| b_b + |b| b_a``; ``a / b`` carries
  ``b_a / |b| + |a / b| b_b / |b|``; ``exp`` / ``log1p`` carry the argument's budget times the
  derivative plus ``FN_ULPS`` roundings (``expf`` / ``log1pf`` are within one ulp);
* a sum of n terms on a tree of depth d carries the terms' budgets plus ``d * sum|x|``.  The depths
  are the kernels': a 64-lane wave reduction or suffix scan is 6 levels deep; a per-lane running sum
  over the ray's rows adds one level per row (``rows + 6`` for colour, alpha and the suffix sums
  behind ``Q``); the loss sums add the per-wave ray loop, the 4-wave workgroup pair tree and the
  final per-lane loop over the workgroup partials;
* a product of n factors (the exclusive transmittance ``T``) is rounded at most n times whatever
  its tree, so ``b_T = T (n + sum_k b_tau_k / tau_k)``, n counting the factors that are not exactly 1.

``sum|terms|`` of the last operation alone would not do: f32 ``alpha = 1 - e`` rounds to the 2^-24
grid, so ``u = (1 - alpha) + 1e-10`` keeps none of ``e``'s low bits behind a surface.  For
``e < 1/2`` the reference therefore emulates that step exactly: ``1 - alpha32 = k 2^-24`` with
``k = round(e32 / 2^-24)``, and ``u32 = fl(k 2^-24 + 1e-10f)``, k being taken from ``e`` and its budget
(both neighbours, the budget covering the pair, when ``e``'s budget reaches a rounding midpoint).
For ``e >= 1/2`` the subtraction is exact and ``u32 = e32``.

Branches follow the kernel's f32 decisions, as the MLP reference follows the kernel's ReLU mask:

* ``tau = min(u, 1)``: the gradient ``dtau/du`` is 1 below the clamp, 1/2 on a tie, 0 above it.
  ``u32 == 1`` exactly when ``expf(-x) == 1`` (``x = sigma delta``), so the tie holds for
  ``|x| < 2^-26``; ``x > 2^-23`` is certainly below, ``x < -2^-22`` certainly above.  In the windows
  between, either branch is accepted: ``dtau/du`` is the midpoint of the two and half their difference
  enters the budget.
* softplus switches to the identity at ``logit > 20`` (threshold of ``F.softplus``).
* depth: the pick is the first index whose weight is the largest among the inner samples, unless
  ``alpha < 0.1f`` (then the last sample).  ``check_depth`` accepts a pick that some f32 weights
  within budget could have produced, and either decision of ``alpha < 0.1f`` when alpha's budget
  reaches 0.1f; ``t[pick]`` must match exactly.

Teeth: every comparison is repeated against references with one deliberate change (``TEETH``), which
the kernel's output must then fail.  Each change must touch some element of the data and exceed the
bound there (``teeth_status``).
"""

import math

import numpy as np
import torch

U = 2.0 ** -24
TINY = 2.0 ** -126           # a rounding in the denormal range (2^-150 absolute), in units of U
FN_ULPS = 2.0                # expf / log1pf: within 1 ulp = 2u relative
DECIDE = 4.0                 # safety factor on a budget that decides a rounding (the 2^-24 grid of alpha)
TIE_BELOW, TIE_ABOVE = 2.0 ** -23, -2.0 ** -22     # x beyond these: certainly below / above the clamp
TIE_SURE = 2.0 ** -26                              # |x| below this: certainly a tie (expf(-x) == 1)
EPS10 = float(np.float32(1e-10))
ALPHA_CUT = float(np.float32(0.1))
WAVE = 6                     # levels of a 64-lane reduction / scan

# kappa per output, fixed.  Measured on an MI355X over every case of tests/test_composite_reference_gpu.py
# (exact f32 and bf16x6 run the same composite) and set to about twice the worst ratio
# |err| / (2^-24 budget) seen, which is given after each value.  The budget is a worst case of every
# rounding at once, so the ratios stay at or below 1.
KAPPA = dict(colour=1.6,         # [0.772]
             alpha=0.6,          # [0.272]
             weights=2.0,        # [0.998]
             d_sigma=2.0,        # [1.000]
             d_t=2.0,            # [1.000]
             d_logits=2.0,       # [1.000]  (all four columns)
             loss_sums=0.6,      # [0.305]  (K6 sums, K5t partials, loss_from_partials sums)
             d_colour=1.8,       # [0.868]  (K6 d_colour and d_alpha)
             loss=0.8)           # [0.374]  (loss_from_partials, loss_value)

# the deliberate changes of the reference
TEETH = ("tie_rule", "last_in_alpha", "no_eps", "inclusive_T", "q_own_term", "last_delta", "dropped_sample")
TEETH_DOC = dict(tie_rule="dtau/du = 1 instead of 1/2 on a tie",
                 last_in_alpha="the last sample counted in alpha and given d_alpha",
                 no_eps="u = 1 - alpha (the 1e-10 dropped)",
                 inclusive_T="inclusive instead of exclusive transmittance",
                 q_own_term="Q includes the sample's own g w",
                 last_delta="the last delta 0 instead of 1e10",
                 dropped_sample="one sample's g w missing from the Q of the samples before it")


def f32(x):
    return float(np.float32(x))


class V:
    """A float64 value ``v`` and the error budget ``b`` (units of U) of its f32 evaluation."""

    __slots__ = ("v", "b")

    def __init__(self, v, b=None):
        self.v = v
        self.b = torch.zeros_like(v) if b is None else b

    @staticmethod
    def rounded(v, b):
        return V(v, b + v.abs() + TINY)

    @staticmethod
    def _parts(o):
        return (o.v, o.b) if isinstance(o, V) else (o, 0.0)

    def __add__(self, o):
        ov, ob = V._parts(o)
        return V.rounded(self.v + ov, self.b + ob)

    __radd__ = __add__

    def __sub__(self, o):
        ov, ob = V._parts(o)
        return V.rounded(self.v - ov, self.b + ob)

    def __rsub__(self, o):
        ov, ob = V._parts(o)
        return V.rounded(ov - self.v, self.b + ob)

    def __neg__(self):
        return V(-self.v, self.b)

    def exact_mul(self, o):
        """Product without its own rounding (inside an fma, or by 1 / 1/2 / 0)."""
        ov, ob = V._parts(o)
        ov_abs = ov.abs() if isinstance(ov, torch.Tensor) else abs(ov)
        return V(self.v * ov, self.v.abs() * ob + ov_abs * self.b)

    def __mul__(self, o):
        p = self.exact_mul(o)
        return V.rounded(p.v, p.b)

    __rmul__ = __mul__

    def __truediv__(self, o):
        ov, ob = V._parts(o)
        q = self.v / ov
        ov_abs = ov.abs() if isinstance(ov, torch.Tensor) else abs(ov)
        return V.rounded(q, self.b / ov_abs + q.abs() * ob / ov_abs)

    def __rtruediv__(self, c):
        q = c / self.v
        return V.rounded(q, q.abs() * self.b / self.v.abs())

    def exp(self):
        y = torch.exp(self.v)
        return V(y, y * self.b + FN_ULPS * y + TINY)

    def log1p(self):
        y = torch.log1p(self.v)
        return V(y, self.b / (1.0 + self.v) + FN_ULPS * y.abs() + TINY)

    def __getitem__(self, idx):
        return V(self.v[idx], self.b[idx])

    @staticmethod
    def where(cond, a, b):
        av, ab = V._parts(a)
        bv, bb = V._parts(b)
        return V(torch.where(cond, torch.as_tensor(av, dtype=torch.float64, device=cond.device),
                             torch.as_tensor(bv, dtype=torch.float64, device=cond.device)),
                 torch.where(cond, torch.as_tensor(ab, dtype=torch.float64, device=cond.device),
                             torch.as_tensor(bb, dtype=torch.float64, device=cond.device)))

    @staticmethod
    def stack(vs, dim):
        return V(torch.stack([x.v for x in vs], dim), torch.stack([x.b for x in vs], dim))


def vsum(x, dim, depth):
    """Sum over ``dim`` on a tree of depth ``depth``."""
    n = x.v.shape[dim]
    return V(x.v.sum(dim), x.b.sum(dim) + depth * x.v.abs().sum(dim) + n * TINY)


def sigmoid(x):
    return 1.0 / (1.0 + (-x).exp())


def softplus(x):
    """F.softplus (threshold 20) of the exact logits ``x`` (float64 tensor)."""
    lg = V(x)
    return V.where(x > 20.0, lg, lg.exp().log1p())


def rows_of(S):
    return (S + 63) // 64


# ------------------------------------------------------------------------------------- weights
def _delta(t, variant):
    """delta_s = t_{s+1} - t_s, the last 1e10 (exact f32 inputs)."""
    d = V.rounded(t[:, 1:] - t[:, :-1], torch.zeros_like(t[:, 1:]))
    last = 0.0 if variant == "last_delta" else 1e10
    col = torch.full_like(t[:, :1], last)
    return V(torch.cat([d.v, col], 1), torch.cat([d.b, torch.zeros_like(col)], 1))


def _u_grid(k, eps):
    """u32 = fl(k 2^-24 + 1e-10f), k < 2^23 (an exact f32 evaluation on the host)."""
    u = k.float() * (2.0 ** -24)
    if eps:
        u = u + torch.tensor(EPS10, dtype=torch.float32, device=k.device)
    return u.double()


def weights(sigma, delta, variant=None):
    """Terms of ``alpha_s = 1 - exp(-sigma_s delta_s)``, ``tau_s = min(1, (1 - alpha_s) + 1e-10)``,
    ``T_s = prod_{k<s} tau_k``, ``w_s = alpha_s T_s``.  ``sigma`` / ``delta``: V (R, S)."""
    R, S = sigma.v.shape
    x = sigma * delta
    e = (-x).exp()
    alpha = 1.0 - e
    xv, ev = x.v, e.v
    # u = (1 - alpha) + 1e-10 as the kernel rounds it (module docstring)
    hi = ev >= 0.5
    slack = DECIDE * U * e.b
    k_lo = torch.round((ev - slack).clamp(0.0, 0.5) * 2.0 ** 24)
    k_hi = torch.round((ev + slack).clamp(0.0, 0.5) * 2.0 ** 24)
    eps = variant != "no_eps"
    u_lo, u_hi = _u_grid(k_lo, eps), _u_grid(k_hi, eps)
    # (next to 1/2, e32 and the grid value differ by up to 2^-25: half a unit either way)
    near_half = (ev - 0.5).abs() < 2.0 ** -20 + DECIDE * U * e.b
    grid = V((u_lo + u_hi) * 0.5, (u_hi - u_lo) * (0.5 / U) + torch.where(near_half, 0.5, 0.0))
    u = V.where(hi, V(ev, e.b + torch.where(near_half, 0.5, 0.0)), grid)
    # the clamp's branch, from x: 1 below, 1/2 on a tie, 0 above; the windows take either
    below, tie, above = xv > TIE_BELOW, xv.abs() < TIE_SURE, xv < TIE_ABOVE
    window = ~(below | tie | above)
    tie_value = 1.0 if variant == "tie_rule" else 0.5
    mid = torch.where(below, 1.0, torch.where(tie, tie_value, torch.where(above, 0.0,
                                                                          torch.where(xv > 0, 0.75, 0.25))))
    dtau = V(mid, torch.where(window, 0.25 / U, 0.0))
    # on a certain tie or above the clamp the kernel's tau is exactly 1: what is left is how far the
    # float64 value lies from 1
    one = hi & (tie | above)
    tau_v = torch.where(hi, u.v.clamp_max(1.0), u.v)
    tau = V(tau_v, torch.where(one, (1.0 - tau_v) / U, u.b) + torch.where(hi & window, (1.0 - u.v).abs() / U, 0.0))
    # T: exclusive (inclusive for the tooth) product; n = factors the kernel does not hold as exactly 1
    ones = torch.ones_like(tau.v[:, :1])
    zeros = torch.zeros_like(ones)
    rounded = (~one).double()
    rel = torch.where(tau.v > 0, tau.b / tau.v.abs().clamp_min(1e-300), 0.0) + rounded
    if variant == "inclusive_T":
        Tv, n, cnt = torch.cumprod(tau.v, 1), torch.cumsum(rel, 1), torch.cumsum(rounded, 1)
    else:
        Tv = torch.cumprod(torch.cat([ones, tau.v[:, :-1]], 1), 1)
        n = torch.cumsum(torch.cat([zeros, rel[:, :-1]], 1), 1)
        cnt = torch.cumsum(torch.cat([zeros, rounded[:, :-1]], 1), 1)
    T = V(Tv, Tv * n + cnt * TINY)
    w = alpha * T
    return dict(delta=delta, x=x, e=e, alpha=alpha, tau=tau, dtau=dtau, T=T, w=w)


def _suffix_excl(v):
    """sum_{k > s} along dim 1."""
    inc = v.flip(1).cumsum(1).flip(1)
    return torch.cat([inc[:, 1:], torch.zeros_like(inc[:, :1])], 1)


def _dropped_index(gw):
    """Per ray, the sample (s >= 1) with the largest |g w|: the sample the tooth drops."""
    a = gw.abs().clone()
    a[:, 0] = -1.0
    return a.argmax(1, keepdim=True)


def dL_dalpha(wt, g, variant=None):
    """``dL/dalpha_s = g_s T_s - dtau/du Q_s / tau_s`` (s < S-1; ``g_s T_s`` for the last sample) with
    ``Q_s = sum_{k>s} g_k w_k`` (composite.hip, blend_weights_bwd_kernel)."""
    R, S = g.v.shape
    gw = g * wt["w"]
    depth = WAVE + rows_of(S)
    # the kernel forms Q as (suffix sum including the own term) - own term + tail: the rounding of the
    # suffix sum counts every term at or after s, the own term included (the cancellation)
    Qv = _suffix_excl(gw.v)
    if variant == "q_own_term":
        Qv = Qv + gw.v
    if variant == "dropped_sample" and S > 1:
        k = _dropped_index(gw.v)
        s = torch.arange(S, device=g.v.device)[None]
        Qv = Qv - torch.where(s < k, gw.v.gather(1, k), 0.0)
    Q = V(Qv, _suffix_excl(gw.b) + depth * (_suffix_excl(gw.v.abs()) + gw.v.abs()) + 2 * Qv.abs() + S * TINY)
    inner = torch.arange(S, device=g.v.device)[None] < S - 1
    dtau = Q / wt["tau"]
    dtau = V(torch.where(inner, dtau.v, 0.0), torch.where(inner, dtau.b, 0.0))
    return g * wt["T"] - wt["dtau"].exact_mul(dtau)


# ------------------------------------------------------------------------------------- composite
def composite_forward(logits, t, variant=None):
    """K5 of (R, S, 4) f32 logits and (R, S) f32 t (any device): dict of V colour (R, 3), alpha (R),
    the weights (R, S) and the terms the backward needs."""
    lg = logits.double()
    tt = t.double()
    R, S = tt.shape
    rgb = [sigmoid(V(lg[..., c])) for c in range(3)]
    sigma = softplus(lg[..., 3])
    wt = weights(sigma, _delta(tt, variant), variant)
    w = wt["w"]
    depth = rows_of(S) + WAVE
    colour = V.stack([vsum(w.exact_mul(c), 1, depth) for c in rgb], 1)
    inner = torch.arange(S, device=tt.device)[None] < (S if variant == "last_in_alpha" else S - 1)
    w_in = V(torch.where(inner, w.v, 0.0), torch.where(inner, w.b, 0.0))
    alpha = vsum(w_in, 1, depth)
    return dict(rgb=rgb, sigma=sigma, logit_w=lg[..., 3], wt=wt, colour=colour, alpha=alpha,
                S=S, variant=variant)


def composite_backward(fwd, d_colour, d_alpha):
    """K5b: d_logits (R, S, 4) as V from d_colour (R, 3) and d_alpha (R) (V or exact tensors)."""
    variant = fwd["variant"]
    dc = [d_colour[:, c] if isinstance(d_colour, V) else V(d_colour[:, c].double()) for c in range(3)]
    da = d_alpha if isinstance(d_alpha, V) else V(d_alpha.double())
    S = fwd["S"]
    rgb, wt = fwd["rgb"], fwd["wt"]
    inner = torch.arange(S, device=da.v.device)[None] < (S if variant == "last_in_alpha" else S - 1)
    col = (V(dc[0].v[:, None], dc[0].b[:, None]) * rgb[0] + V(dc[1].v[:, None], dc[1].b[:, None]) * rgb[1]) \
        + V(dc[2].v[:, None], dc[2].b[:, None]) * rgb[2]
    da_s = V(torch.where(inner, da.v[:, None], 0.0), torch.where(inner, da.b[:, None], 0.0))
    g = col + da_s
    dla = dL_dalpha(wt, g, variant)
    d_sigma = (dla * wt["e"]) * wt["delta"]
    x = fwd["logit_w"]
    z = V(x).exp()
    dsig = V.where(x > 20.0, V(torch.ones_like(x)), z / (z + 1.0))
    w = wt["w"]
    outs = [((w * V(dc[c].v[:, None], dc[c].b[:, None])) * rgb[c]) * (1.0 - rgb[c]) for c in range(3)]
    outs.append(d_sigma * dsig)
    return V.stack(outs, 2)


# ------------------------------------------------------------------------------------- blend weights
def blend_forward(t, sigma, variant=None):
    tt = t.double()
    wt = weights(V(sigma.double()), _delta(tt, variant), variant)
    return wt


def blend_backward(wt, sigma, d_weights, variant=None):
    """K5w backward: (d_sigma, d_t) as V from exact d_weights (R, S)."""
    S = sigma.shape[1]
    sg = V(sigma.double())
    dla = dL_dalpha(wt, V(d_weights.double()), variant)
    d_sigma = (dla * wt["e"]) * wt["delta"]
    dd = (dla * wt["e"]) * sg
    inner = torch.arange(S, device=sg.v.device)[None] < S - 1
    dd = V(torch.where(inner, dd.v, 0.0), torch.where(inner, dd.b, 0.0))
    prev = V(torch.cat([torch.zeros_like(dd.v[:, :1]), dd.v[:, :-1]], 1),
             torch.cat([torch.zeros_like(dd.b[:, :1]), dd.b[:, :-1]], 1))
    return d_sigma, prev - dd


# ------------------------------------------------------------------------------------- loss
def mse_rays(colour, alpha, gt_c, gt_a, color_scale, alpha_scale):
    """K6 of one ray each (image_dataset.py:224-262): (ec (R), ea (R) | None, d_colour (R, 3),
    d_alpha (R)) as V.  ``colour`` / ``alpha``: V or exact tensors; ``gt_c`` (R, 3) / ``gt_a`` (R) | None:
    the gathered ground truth."""
    colour = colour if isinstance(colour, V) else V(colour.double())
    alpha = alpha if isinstance(alpha, V) else V(alpha.double())
    gt_c = gt_c.double()
    if gt_a is not None:
        gt_c = torch.where(gt_a[:, None] > 0, gt_c, 0.0)
    d = [colour[:, c] - gt_c[:, c] for c in range(3)]
    ec = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    cs2 = 2.0 * f32(color_scale)                       # exact in f32
    d_colour = V.stack([d[c] * cs2 for c in range(3)], 1)
    if gt_a is None:
        return ec, None, d_colour, V(torch.zeros_like(alpha.v))
    diff = alpha - gt_a.double()
    return ec, diff * diff, d_colour, diff * (2.0 * f32(alpha_scale))


def sum_exact_inputs(x, depth):
    """Sum of exact f32 inputs (a kernel's own partials) on a tree of depth ``depth``."""
    return vsum(V(x.double()), 0, depth)


def k6_depth(R):
    """wave_sum, the workgroup pair tree, the final per-lane loop over the workgroups, wave_sum."""
    blocks = (R + 255) // 256
    return WAVE + 2 + -(-blocks // 64) + WAVE


def train_blocks(R):
    """ray_grid of composite.hip: four rays (waves) per workgroup, at most 4096 workgroups."""
    return max(1, min((R + 3) // 4, 4096))


def partials_of(ec, R):
    """K5t's per-workgroup sums of the per-ray ``ec`` (V (R)): wave w takes rays w, w + waves, ...;
    its lane 0 adds them one by one, then the workgroup's four waves pair up."""
    blocks = train_blocks(R)
    waves = 4 * blocks
    block_of = (torch.arange(R, device=ec.v.device) % waves) // 4
    v = torch.zeros(blocks, dtype=torch.float64, device=ec.v.device).index_add_(0, block_of, ec.v)
    a = torch.zeros_like(v).index_add_(0, block_of, ec.v.abs())
    b = torch.zeros_like(v).index_add_(0, block_of, ec.b)
    depth = -(-R // waves) + 2
    return V(v, b + depth * a + 8 * TINY)


def partials_depth(blocks):
    """loss_from_partials: a per-lane loop over the workgroups, then wave_sum."""
    return -(-blocks // 64) + WAVE


def loss_of(sums, rays, alpha_weight):
    """sums[0] / (3 rays) + alpha_weight * (sums[1] / rays) from exact f32 sums (image_dataset.py:237-242)."""
    s = sums.double()
    colour = V(s[0:1]) / f32(3.0 * rays)
    if f32(alpha_weight) == 0.0:
        return colour + 0.0
    return colour + (V(s[1:2]) / f32(rays)) * f32(alpha_weight)


# ------------------------------------------------------------------------------------- checking
class Report:
    """Worst ratio per output, failures, and the teeth."""

    def __init__(self, kappa=None, teeth_doc=None):
        self.kappa = KAPPA if kappa is None else kappa
        self.teeth_doc = TEETH_DOC if teeth_doc is None else teeth_doc
        self.worst = {}
        self.failures = []
        self.teeth = {}      # tooth -> dict(touched, exceeds, ratio (|got - alt| / bound, worst), out)

    def compare(self, out, key, got, ref):
        """``got``: tensor, ``ref``: V of the same number of elements."""
        got = got.double().reshape(-1).to(ref.v.device)
        rv, rb = ref.v.reshape(-1), ref.b.reshape(-1)
        if got.numel() == 0:
            return
        err = (got - rv).abs()
        scale = U * rb
        ok = err <= self.kappa[out] * scale                      # (NaN fails)
        ratio = torch.where(err == 0, torch.zeros_like(err), err / scale)
        ratio = torch.nan_to_num(ratio, nan=float("inf"))
        self.worst[out] = max(self.worst.get(out, 0.0), float(ratio.max()))
        if not bool(ok.all()):
            bad = int((~ok).nonzero()[0, 0])
            self.failures.append("%s %s: %d of %d elements out of bound, first at flat index %d: got %r want %r "
                                 "(bound %.3g)" % (out, key, int((~ok).sum()), ok.numel(), bad, float(got[bad]),
                                                   float(rv[bad]), float(self.kappa[out] * scale[bad])))

    def tooth(self, out, name, got, ref, alt):
        """Records how far the kernel's ``got`` is from the changed reference ``alt``, in units of the
        bound of ``ref``, over the elements the change touches."""
        got = got.double().reshape(-1).to(ref.v.device)
        rv, rb, av = ref.v.reshape(-1), ref.b.reshape(-1), alt.v.reshape(-1)
        touched = ~(av == rv)
        if not bool(touched.any()):
            return
        bound = self.kappa[out] * U * rb[touched]
        shift = (av - rv).abs()[touched]
        exceeds = bool(((shift > bound) | torch.isnan(shift)).any())
        far = torch.nan_to_num((got[touched] - av[touched]).abs() / bound, nan=float("inf"))
        r = float(far.max())
        t = self.teeth.setdefault(name, dict(touched=True, exceeds=False, ratio=0.0, out=None))
        t["exceeds"] = t["exceeds"] or exceeds
        if r > t["ratio"]:
            t["ratio"], t["out"] = r, out

    def problems(self, required_teeth=()):
        p = list(self.failures)
        for name in required_teeth:
            if name not in self.teeth:
                p.append("tooth %s (%s): the data has no element it changes" % (name, self.teeth_doc.get(name, "")))
        for name, t in self.teeth.items():
            if not t["exceeds"]:
                p.append("tooth %s: the changed reference stays within the bound everywhere" % name)
            if not t["ratio"] > 1.0:
                p.append("tooth %s: the kernel passes the changed reference too (worst %.3g of the bound)"
                         % (name, t["ratio"]))
        return p


def depth_candidates(fwd, inner=None):
    """(R, S) bool: the samples whose t the kernel may report as depth (module docstring).
    ``inner`` (R, S) bool: the samples that compete for the pick, by default all but the last (the
    fused render under an occupancy grid lets only its kept samples compete); a ray none of whose
    samples competes reports the last sample whatever its alpha."""
    w, a = fwd["wt"]["w"], fwd["alpha"]
    R, S = w.v.shape
    s = torch.arange(S, device=w.v.device)[None]
    if inner is None:
        inner = s < S - 1
    none_inner = ~inner.any(1, keepdim=True)            # (default: S == 1)
    beta = KAPPA["weights"] * U * w.b
    lo = torch.where(inner, w.v - beta, -math.inf)
    hi = torch.where(inner, w.v + beta, -math.inf)
    top = lo.max(1, keepdim=True).values
    before = torch.cat([torch.full_like(lo[:, :1], -math.inf), torch.cummax(lo, 1).values[:, :-1]], 1)
    argmax = inner & (hi >= top) & (before <= hi)
    beta_a = KAPPA["alpha"] * U * a.b
    surely_below = (a.v + beta_a < ALPHA_CUT)[:, None]
    surely_above = (a.v - beta_a >= ALPHA_CUT)[:, None]
    last = (s == S - 1) & (~surely_above | none_inner)
    return (argmax & ~surely_below) | last


def check_depth(rep, key, fwd, t, depth):
    ok_at = depth_candidates(fwd) & (t.double().to(depth.device) == depth.double()[:, None])
    ok = ok_at.any(1)
    if not bool(ok.all()):
        bad = int((~ok).nonzero()[0, 0])
        rep.failures.append("depth %s: %d of %d rays report a t no candidate sample has, first ray %d: %r"
                            % (key, int((~ok).sum()), ok.numel(), bad, float(depth[bad])))


# ------------------------------------------------------------------------------------- kernels
def measure_composite(rep, key, logits, t, d_colour, d_alpha, colour, alpha, depth, d_logits, teeth=True):
    """K5 (colour, alpha, depth) and K5b (d_logits) of one batch; d_colour / d_alpha exact inputs."""
    for variant in (None,) + (TEETH if teeth else ()):
        fwd = composite_forward(logits, t, variant)
        dl = composite_backward(fwd, d_colour, d_alpha)
        if variant is None:
            ref = (fwd, dl)
            rep.compare("colour", key, colour, fwd["colour"])
            rep.compare("alpha", key, alpha, fwd["alpha"])
            rep.compare("d_logits", key, d_logits, dl)
            if depth is not None:
                check_depth(rep, key, fwd, t, depth)
            continue
        rep.tooth("colour", variant, colour, ref[0]["colour"], fwd["colour"])
        rep.tooth("alpha", variant, alpha, ref[0]["alpha"], fwd["alpha"])
        rep.tooth("d_logits", variant, d_logits, ref[1], dl)


def measure_blend(rep, key, t, sigma, d_weights, w, d_sigma, d_t, teeth=True):
    """K5w (weights) and its backward (d_sigma, d_t; either may be None)."""
    for variant in (None,) + (TEETH if teeth else ()):
        wt = blend_forward(t, sigma, variant)
        back = blend_backward(wt, sigma, d_weights, variant) if d_sigma is not None else None
        if variant is None:
            ref = (wt, back)
            if w is not None:
                rep.compare("weights", key, w, wt["w"])
            if back is not None:
                rep.compare("d_sigma", key, d_sigma, back[0])
                if d_t is not None:
                    rep.compare("d_t", key, d_t, back[1])
            continue
        if w is not None:
            rep.tooth("weights", variant, w, ref[0]["w"], wt["w"])
        if back is not None:
            rep.tooth("d_sigma", variant, d_sigma, ref[1][0], back[0])
            if d_t is not None:
                rep.tooth("d_t", variant, d_t, ref[1][1], back[1])


def measure_mse(rep, key, colour, alpha, gt_colors, gt_alphas, ray_index, color_scale, alpha_scale,
                sums, d_colour, d_alpha):
    """K6 on exact colour / alpha inputs."""
    R = colour.shape[0]
    gc = gt_colors[ray_index]
    ga = None if gt_alphas is None else gt_alphas[ray_index].double()
    ec, ea, dc, da = mse_rays(colour, alpha, gc, ga, color_scale, alpha_scale)
    depth = k6_depth(R)
    rep.compare("loss_sums", key + " colour", sums[0:1], vsum(ec, 0, depth))
    if ea is not None:
        rep.compare("loss_sums", key + " alpha", sums[1:2], vsum(ea, 0, depth))
    rep.compare("d_colour", key, d_colour, dc)
    rep.compare("d_colour", key + " d_alpha", d_alpha, da)


def measure_train(rep, key, logits, t, gt_colors, gt_alphas, ray_index, color_scale, alpha_scale,
                  d_logits, partials, teeth=True):
    """K5t: d_logits and the per-workgroup partials (blocks, 2)."""
    R, S = t.shape
    gc = gt_colors[ray_index]
    ga = None if gt_alphas is None else gt_alphas[ray_index].double()
    for variant in (None,) + (TEETH if teeth else ()):
        fwd = composite_forward(logits, t, variant)
        ec, ea, dc, da = mse_rays(fwd["colour"], fwd["alpha"], gc, ga, color_scale, alpha_scale)
        dl = composite_backward(fwd, dc, da)
        pc = partials_of(ec, R)
        pa = partials_of(ea, R) if ea is not None else None
        if variant is None:
            ref = (dl, pc, pa)
            rep.compare("d_logits", key + " K5t", d_logits, dl)
            rep.compare("loss_sums", key + " K5t colour partials", partials[:, 0], pc)
            if pa is not None:
                rep.compare("loss_sums", key + " K5t alpha partials", partials[:, 1], pa)
            else:
                if not bool((partials[:, 1] == 0).all()):
                    rep.failures.append("%s K5t: alpha partials not 0 without ground-truth alpha" % key)
            continue
        rep.tooth("d_logits", variant, d_logits, ref[0], dl)
        rep.tooth("loss_sums", variant, partials[:, 0], ref[1], pc)
        if pa is not None:
            rep.tooth("loss_sums", variant, partials[:, 1], ref[2], pa)


def measure_loss(rep, key, partials, rays, alpha_weight, sums, loss, loss2):
    """loss_from_partials (sums, loss) from the kernel's own partials; loss_value (``loss2``) from
    the kernel's own sums."""
    depth = partials_depth(partials.shape[0])
    rep.compare("loss_sums", key + " from partials colour", sums[0:1], sum_exact_inputs(partials[:, 0], depth))
    rep.compare("loss_sums", key + " from partials alpha", sums[1:2], sum_exact_inputs(partials[:, 1], depth))
    ref = loss_of(sums, rays, alpha_weight)
    rep.compare("loss", key + " loss_from_partials", loss.reshape(1), ref)
    rep.compare("loss", key + " loss_value", loss2.reshape(1), ref)


# ------------------------------------------------------------------------------------- data
REGIMES = ("transparent", "surface", "dense", "duplicate_t", "thresholds", "random", "negative")


def _inv_softplus(sigma):
    return torch.where(sigma > 20.0, sigma, torch.log(torch.expm1(sigma.clamp_min(1e-30))))


def make_rays(R, S, seed):
    """(logits (R, S, 4), t (R, S), sigma (R, S)) f32 on the CPU; ray r is in regime
    ``REGIMES[(r + seed) % len(REGIMES)]``:

    * transparent: sigma logits in [-40, -22] (x far below 2^-26: ties) or [-8, -2];
    * surface: one sample with x = sigma delta in [5, 40], a thin medium around it;
    * dense: x in [1.5, 4] at every sample, T falling through the denormals to 0;
    * duplicate_t: t in equal pairs (delta = 0);
    * thresholds: sigma logits at 20, at 20 plus one ulp, in [-104, -88], or random;
    * random: randn logits;
    * negative: negative opacity at every sample but the last (``sigma`` only: blend weights).

    ``sigma`` is softplus(logits) except in the negative regime."""
    g = torch.Generator().manual_seed(seed)

    def rnd(*shape):
        return torch.rand(*shape, generator=g, dtype=torch.float64)

    def nrm(*shape):
        return torch.randn(*shape, generator=g, dtype=torch.float64)

    regime = (torch.arange(R) + seed) % len(REGIMES)
    t = (2.0 + rnd(R, 1) + torch.sort(rnd(R, S), 1).values * 4.0).float().double()
    dup = regime == REGIMES.index("duplicate_t")
    if S > 1:
        td = t.clone()
        td[:, 1::2] = t[:, 0:S - 1:2][:, :td[:, 1::2].shape[1]]
        t = torch.where(dup[:, None], td, t)
    delta = torch.cat([t[:, 1:] - t[:, :-1], torch.full_like(t[:, :1], 1e10)], 1).clamp_min(1e-6)
    lg = nrm(R, S, 4) * 3.0
    w = nrm(R, S) * 2.0
    pick = rnd(R, S)
    trans = torch.where(pick < 0.5, -22.0 - 18.0 * rnd(R, S), -2.0 - 6.0 * rnd(R, S))
    w = torch.where((regime == REGIMES.index("transparent"))[:, None], trans, w)
    surf = -2.0 - 4.0 * rnd(R, S)
    if S > 1:
        j = (rnd(R) * (S - 1)).long().clamp_max(S - 2)
        xs = 5.0 + 35.0 * rnd(R)
        at = torch.arange(S)[None] == j[:, None]
        surf = torch.where(at, _inv_softplus(xs[:, None] / delta), surf)
    w = torch.where((regime == REGIMES.index("surface"))[:, None], surf, w)
    dense = _inv_softplus((1.5 + 2.5 * rnd(R, S)) / delta)
    w = torch.where((regime == REGIMES.index("dense"))[:, None], dense, w)
    up = float(np.nextafter(np.float32(20.0), np.float32(np.inf)))
    thr = torch.where(pick < 0.25, 20.0, torch.where(pick < 0.5, up, torch.where(
        pick < 0.75, -88.0 - 16.0 * rnd(R, S), w)))
    w = torch.where((regime == REGIMES.index("thresholds"))[:, None], thr, w)
    lg[..., 3] = w
    logits = lg.float()
    sigma = torch.nn.functional.softplus(logits[..., 3])
    neg = -2.0 * rnd(R, S).float()
    neg[:, -1] = sigma[:, -1]
    sigma = torch.where((regime == REGIMES.index("negative"))[:, None], neg, sigma)
    return logits.contiguous(), t.float().contiguous(), sigma.contiguous()


def make_grads(R, S, seed):
    """(d_colour (R, 3), d_alpha (R), d_weights (R, S)) f32: ordinary, zero or large, rotating
    independently of the ray regimes."""
    g = torch.Generator().manual_seed(seed + 1)
    r = torch.arange(R)
    mag = torch.tensor([1.0 / (3 * max(R, 1)), 0.0, 1e3], dtype=torch.float64)
    dc = torch.randn(R, 3, generator=g, dtype=torch.float64) * mag[(r // 7) % 3][:, None]
    da = torch.randn(R, generator=g, dtype=torch.float64) * mag[(r // 3) % 3] * 0.1
    dw = torch.randn(R, S, generator=g, dtype=torch.float64) * mag[(r // 5) % 3][:, None]
    return dc.float(), da.float(), dw.float()


def make_truth(R, seed):
    """(gt_colors (N, 3), gt_alphas (N), ray_index (R)) with N = R + 5; ground-truth alpha 0, 1 or in
    between."""
    g = torch.Generator().manual_seed(seed + 2)
    N = R + 5
    gc = torch.rand(N, 3, generator=g)
    ga = torch.rand(N, generator=g)
    sel = torch.arange(N) % 3
    ga = torch.where(sel == 0, 0.0, torch.where(sel == 1, 1.0, ga))
    return gc, ga, torch.randperm(N, generator=g)[:R]
