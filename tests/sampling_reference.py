"""Float64 reference of the ray front end (csrc/rays.hip, csrc/focus.hip, csrc/focus_terms.h) with a
first-order error budget for every output element.

What is checked, on the kernels' own f32 inputs:

* K1   ``ffn_raygen_nearfar``       directions, starts, near/far, valid   (camera_info.py:99-109,
                                                                           ray_sampler.py:202-232)
* K2a  ``ffn_sample_t``             t                                      (ray_sampler.py:373-386)
* K2b  ``ffn_materialise_samples``  positions, views
* K2ab ``ffn_sample_materialise``   t, positions, views
* K2c  ``ffn_cdf_build`` / ``ffn_cdf_build_logits``  the CDF rows         (ray_sampler.py:59-67)
* K2d  ``ffn_focus_sample_merge`` (table and ``_rows`` forms)  the merged, sorted t rows
                                                                           (ray_sampler.py:301-357)

Budgets are carried by ``composite_reference.V`` (value + first-order bound in units of 2^-24) and an
element passes when ``|got - ref| <= kappa * 2^-24 * budget``:

* K1 directions follow the kernel's operations: the fused chain ``w = fma(u3, 1, fma(u2, 1, fma(u1,
  py, u0 px)))`` (one rounding per step), ``world - cam``, ``sqrt((dx dx + dy dy) + dz dz)``, the
  division.  Starts must be ``cam_pos`` exactly.  The slab test is recomputed from the kernel's own
  starts / directions, so a zero direction component gives the same inf / NaN on both sides; min / max
  carry the larger budget of their two arguments (they are 1-Lipschitz), NaN propagates like the
  kernel's ``np_max`` / ``np_min``.  ``valid`` must equal the float64 ``near < far`` wherever
  ``|far - near|`` exceeds its budget (inside that window either answer is accepted); near is clamped
  to 0.1f on the rays the kernel calls valid, and where the float64 near lies below 0.1f by more than
  its budget the kernel's near must be exactly 0.1f.
* K2a/K2b t, positions and views must be bit-identical to the oracle's f32 operation sequence
  (``orc.anneal_range``, ``orc.uniform_t`` with the kernel's own ``unit``, ``start + t dir``) and
  within their float64 budget; positions are checked on the kernel's own t.
* K2c: the blend weights of ``composite_reference.weights`` (alpha exactly 0 on a certain tie, as
  its tau is exactly 1 there), ``+ 1e-5``, an inclusive running sum of
  depth ``sum_depth`` (the kernel: a 6-level wave scan plus one level per 64-sample row) and one
  rounding for the division.  Exact invariants: ``cdf[:, 0] == 0``, the last entry ``== 1.0f``, every
  row non-decreasing (``searchsorted`` relies on it).
* K2d follows the kernel's f32 decisions on its own CDF row: the bin ``k = #(c <= u)`` (right=True),
  ``lo = max(k - 1, 0)``, ``hi = min(k, width - 1)`` and ``denom < 1e-5f`` in f32.  The focus values
  must be bit-identical to ``orc.focus_t`` (with the kernel's ``unit_focus``) and within their
  float64 budget; the written row must be ``torch.sort(cat(uniform_in, focus))`` exactly.  (The
  kernel only writes the sorted row: its focus values are those of ``orc.focus_t`` because the row
  matches bit for bit, and it is those values that the budget and the teeth judge.)

Teeth: every comparison is repeated against references with one deliberate change (``TEETH``); the
kernel's output must fail each, and each must touch some element of the data.
"""

import numpy as np
import torch

from oracle import ffn_oracle as orc
from tests import composite_reference as cr
from tests.composite_reference import FN_ULPS, TINY, U, V, WAVE

NEAR_MIN = float(np.float32(0.1))
EPS5 = float(np.float32(1e-5))
F32_MAX = float(np.finfo(np.float32).max)
ROW = 64                     # probe samples per row of the K2c scan (one per lane)

# kappa per output, fixed.  Measured on an MI355X over every case of tests/test_sampling_reference_gpu.py
# (f32 and bf16x6 run the same sampling kernels) and set to about twice the worst ratio
# |err| / (2^-24 budget) seen, which is given after each value.
KAPPA = dict(dirs=1.8,           # [0.855]
             near_far=1.7,       # [0.827]
             t=2.0,              # [0.976]  (K2a / K2ab t)
             positions=2.0,      # [0.997]  (K2b / K2ab positions)
             cdf=2.0,            # [0.996]  (K2c, both forms and the live path's)
             focus=1.3)          # [0.645]  (K2d focus values, both forms and the live path's)

TEETH = ("near_unclamped", "clamp_before_test", "pixel_centre", "stratified_scale", "anneal_about_near",
         "cdf_first_weight", "cdf_last_weight", "no_eps", "exclusive_sum", "no_carry", "right_false",
         "no_denom_clamp", "bin_edges", "annealed_focus")
TEETH_DOC = dict(near_unclamped="near not clamped to 0.1f",
                 clamp_before_test="near clamped to 0.1f before the validity test",
                 pixel_centre="pixel centres at +0.5",
                 stratified_scale="stratified jitter scaled by span / (count - 1)",
                 anneal_about_near="annealing about near instead of the midpoint",
                 cdf_first_weight="CDF of weights 0 .. n-3 (the first weight in, the last inner one out)",
                 cdf_last_weight="CDF of weights 2 .. n-1 (the last weight in, the first inner one out)",
                 no_eps="CDF without the + 1e-5",
                 exclusive_sum="exclusive instead of inclusive running sum",
                 no_carry="transmittance and running sum restarted at every 64-sample row",
                 right_false="searchsorted(right=False)",
                 no_denom_clamp="no denom < 1e-5 clamp",
                 bin_edges="bin edges instead of bin centres",
                 annealed_focus="the focus half on annealed near / far")
K1_TEETH = ("near_unclamped", "clamp_before_test", "pixel_centre")
K2_TEETH = ("stratified_scale", "anneal_about_near")
CDF_TEETH = ("cdf_first_weight", "cdf_last_weight", "no_eps", "exclusive_sum", "no_carry")
MERGE_TEETH = ("right_false", "no_denom_clamp", "bin_edges", "annealed_focus")
FOCUS_ANNEAL = float(np.float32(0.5))          # the annealing of the annealed_focus tooth


def cdf_teeth(n):
    """The CDF teeth a probe of n samples can show: with n = 3 the one inner weight normalises to
    [0, 1] whatever it is; the row carry needs an inner sample in a second row (n > 65)."""
    if n == 3:
        return ("exclusive_sum",)
    return tuple(x for x in CDF_TEETH if x != "no_carry" or n > ROW + 1)


def merge_teeth(n_focus):
    """The merge teeth n_focus samples can show: right=False moves a sample only where u sits on an
    entry c_j with c_j - c_{j-1} < 1e-5, which the CDF [0, 1] of n_focus = 3 and the [0] of n_focus = 2
    do not have; with one bin (n_focus = 2) every sample is its centre, which annealing keeps."""
    return tuple(x for x in MERGE_TEETH
                 if (x != "right_false" or n_focus > 3) and (x != "annealed_focus" or n_focus > 2))


def new_report():
    return cr.Report(KAPPA, TEETH_DOC)


def _rowsel(x, b):
    return V(x.v[b], x.b[b])


def _sqrt(x):
    y = x.v.sqrt()
    return V(y, x.b / (2.0 * y) + FN_ULPS * y + TINY)


def _finite_budget(x):
    """Non-finite values are exact (inf from x / 0, NaN from 0 / 0, the same on both sides); values
    beyond the f32 range are the kernel's inf."""
    big = x.v.abs() > F32_MAX
    v = torch.where(big & torch.isfinite(x.v), x.v.sign() * float("inf"), x.v)
    return V(v, torch.where(torch.isfinite(v), x.b, 0.0))


def _pick(cond, a, b):
    """where(cond, a, b) with the budget of a 1-Lipschitz selection: the larger of the two where both
    are finite, the chosen one's otherwise."""
    both = torch.isfinite(a.v) & torch.isfinite(b.v)
    v = torch.where(cond, a.v, b.v)
    bb = torch.where(both, torch.maximum(a.b, b.b), torch.where(cond, a.b, b.b))
    return V(v, bb)


def _np_max(a, b):
    nan = torch.isnan(a.v) | torch.isnan(b.v)
    m = _pick(a.v > b.v, a, b)
    return V(torch.where(nan, float("nan"), m.v), torch.where(nan, 0.0, m.b))


def _np_min(a, b):
    nan = torch.isnan(a.v) | torch.isnan(b.v)
    m = _pick(a.v < b.v, a, b)
    return V(torch.where(nan, float("nan"), m.v), torch.where(nan, 0.0, m.b))


# ------------------------------------------------------------------------------------- K1
def pixels(width, height, points=None, device="cpu"):
    """(px, py) float64 per pixel of one camera, in the kernel's ray order."""
    if points is not None:
        p = points.double().to(device)
        return p[:, 0], p[:, 1]
    pix = torch.arange(width * height, device=device)
    return (pix % width).double(), torch.div(pix, width, rounding_mode="floor").double()


def directions(unproj, cam_pos, width, height, points=None, variant=None):
    """V (C * W * H, 3) unit directions of K1 from its f32 inputs ``unproj`` (C, 4, 4), ``cam_pos`` (C, 3)."""
    dev = unproj.device
    px, py = pixels(width, height, points, dev)
    if variant == "pixel_centre":
        px, py = px + 0.5, py + 0.5
    u = unproj.double()
    cam = cam_pos.double()
    d = []
    for k in range(3):
        acc = V.rounded(u[:, k, 0:1] * px[None], torch.zeros(u.shape[0], px.numel(), dtype=torch.float64, device=dev))
        acc = V(u[:, k, 1:2] * py[None]) + acc                   # exact products: each fma rounds once
        acc = acc + u[:, k, 2:3]
        acc = acc + u[:, k, 3:4]
        d.append(acc - cam[:, k:k + 1])
    norm = _sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    r = [x / norm for x in d]
    return V(torch.stack([x.v for x in r], -1).reshape(-1, 3), torch.stack([x.b for x in r], -1).reshape(-1, 3))


def slab(starts, dirs, lo, hi):
    """near, far (V (R,)) of the slab test on the kernel's own f32 ``starts`` / ``dirs`` (R, 3)."""
    s, r = starts.double(), dirs.double()
    lo = torch.as_tensor(np.asarray(lo, np.float32), device=s.device).double()
    hi = torch.as_tensor(np.asarray(hi, np.float32), device=s.device).double()
    near = far = None
    for k in range(3):
        zero = torch.zeros_like(s[:, k])
        a = _finite_budget(V.rounded(lo[k] - s[:, k], zero) / r[:, k])
        b = _finite_budget(V.rounded(hi[k] - s[:, k], zero) / r[:, k])
        # nx = a < b ? a : b, fx = a > b ? a : b (a NaN a gives b, a NaN b gives NaN)
        n_k, f_k = _pick(a.v < b.v, a, b), _pick(a.v > b.v, a, b)
        near = n_k if near is None else _np_max(near, n_k)
        far = f_k if far is None else _np_min(far, f_k)
    return near, far


def check_raygen(rep, key, unproj, cam_pos, width, height, box_lo, box_hi, points, starts, dirs, near_far, valid,
                 teeth=True):
    """K1 of one launch: every output against the float64 reference (module docstring)."""
    C = unproj.shape[0]
    per = width * height
    ref = directions(unproj, cam_pos, width, height, points)
    rep.compare("dirs", key, dirs, ref)
    cam = cam_pos.repeat_interleave(per, 0).to(starts.device)
    if not bool((starts == cam).all()):
        rep.failures.append("starts %s: %d rays do not start at cam_pos exactly" % (key, int((starts != cam).any(1).sum())))
    near, far = slab(starts, dirs, box_lo, box_hi)
    ok = valid.to(near.v.device).bool()
    kappa = rep.kappa["near_far"]
    window = (far.v - near.v).abs() <= kappa * U * (near.b + far.b)
    decided = near.v < far.v
    wrong = (ok != decided) & ~window
    if bool(wrong.any()):
        i = int(wrong.nonzero()[0, 0])
        rep.failures.append("valid %s: %d rays disagree with the float64 slab test outside its window, first %d: "
                            "near %r far %r valid %d" % (key, int(wrong.sum()), i, float(near.v[i]), float(far.v[i]),
                                                         int(ok[i])))
    clamp_ref = V(torch.where(ok, near.v.clamp_min(NEAR_MIN), near.v), near.b)
    _compare_finite(rep, "near_far", key + " near", near_far[0], clamp_ref)
    _compare_finite(rep, "near_far", key + " far", near_far[1], far)
    sure = ok & (near.v + kappa * U * near.b < NEAR_MIN)
    got_near = near_far[0].to(near.v.device)
    if not bool((got_near[sure] == NEAR_MIN).all()):
        rep.failures.append("near_far %s: %d clamped rays have a near other than 0.1f"
                            % (key, int((got_near[sure] != NEAR_MIN).sum())))
    if not teeth:
        return
    alt = directions(unproj, cam_pos, width, height, points, "pixel_centre")
    rep.tooth("dirs", "pixel_centre", dirs, ref, alt)
    fin = torch.isfinite(near.v)
    rep.tooth("near_far", "near_unclamped", near_far[0][fin.to(near_far.device)], _rowsel(clamp_ref, fin), _rowsel(near, fin))
    pre = near.v.clamp_min(NEAR_MIN)
    alt_valid = (pre < far.v) & ~window
    tooth_exact(rep, "clamp_before_test", ok[~window], decided[~window], alt_valid[~window])
    alt_near = V(torch.where(pre < far.v, pre, near.v), near.b)
    rep.tooth("near_far", "clamp_before_test", near_far[0][fin.to(near_far.device)], _rowsel(clamp_ref, fin),
              _rowsel(alt_near, fin))


def _compare_finite(rep, out, key, got, ref):
    got = got.to(ref.v.device)
    fin = torch.isfinite(ref.v)
    rep.compare(out, key, got[fin], _rowsel(ref, fin))
    g, r = got[~fin].double(), ref.v[~fin]
    same = (g == r) | (torch.isnan(g) & torch.isnan(r))
    if not bool(same.all()):
        rep.failures.append("%s %s: %d non-finite reference elements differ" % (out, key, int((~same).sum())))


def tooth_exact(rep, name, got, ref, alt):
    """A tooth of an exact output (flags, bits): the elements ``alt`` changes must differ in ``got``."""
    touched = alt != ref
    if not bool(touched.any()):
        return
    far = float("inf") if bool((got[touched] != alt[touched]).any()) else 0.0
    t = rep.teeth.setdefault(name, dict(touched=True, exceeds=False, ratio=0.0, out=None))
    t["exceeds"] = True
    if far > t["ratio"]:
        t["ratio"], t["out"] = far, "exact"


# ------------------------------------------------------------------------------------- K2a / K2b
def anneal64(near, far, anneal, variant=None):
    if anneal is None:
        return near, far
    mid = near if variant == "anneal_about_near" else (near + far) * 0.5
    return mid + (near - mid) * anneal, mid + (far - mid) * anneal


def uniform_t64(near, far, unit, noise, anneal, variant=None):
    """V (R, count) of K2a from the per-ray f32 near / far (R,), the kernel's ``unit`` (count,),
    ``noise`` (R, count) | None and the f32 ``anneal`` | None."""
    count = unit.numel()
    n, f = anneal64(V(near.double()[:, None]), V(far.double()[:, None]), anneal, variant)
    span = f - n
    t = n + V(unit.double().to(near.device)[None]) * span
    if noise is not None:
        scale = span / float(count - 1 if variant == "stratified_scale" else count)
        t = t + V(noise.double()) * scale
    return t


def uniform_t32(near, far, unit, noise, anneal):
    """The oracle's f32 operation sequence (CPU tensors)."""
    if anneal is not None:
        near, far = orc.anneal_range(near, far, 0, anneal, 1)
    return orc.uniform_t(near, far, unit.numel(), noise, unit)


def positions32(starts, dirs, t):
    R, S = t.shape
    return starts.reshape(R, 1, 3) + t.unsqueeze(-1) * dirs.reshape(R, 1, 3)


def positions64(starts, dirs, t):
    """V (R, S, 3) of K2b on the kernel's own t."""
    s = starts.double()[:, None, :]
    p = V(t.double()[..., None] * dirs.double()[:, None, :])
    return V.rounded(p.v, torch.zeros_like(p.v)) + s


def check_bits(rep, out, key, got, want):
    got = got.to(want.device)
    same = (got == want) | (torch.isnan(got) & torch.isnan(want))
    if not bool(same.all()):
        i = int((~same).reshape(-1).nonzero()[0, 0])
        rep.failures.append("%s %s: %d of %d elements differ from the oracle's f32 sequence, first at flat index %d: "
                            "got %r want %r" % (out, key, int((~same).sum()), same.numel(), i,
                                                float(got.reshape(-1)[i]), float(want.reshape(-1)[i])))


def check_sample_t(rep, key, near, far, unit, noise, anneal, t, teeth=True):
    """K2a / K2ab t of rays with the f32 near / far (R,) (CPU tensors)."""
    check_bits(rep, "t", key, t, uniform_t32(near, far, unit, noise, anneal))
    ref = uniform_t64(near, far, unit, noise, anneal)
    rep.compare("t", key, t, ref)
    if teeth:
        for variant in K2_TEETH:
            alt = uniform_t64(near, far, unit, noise, anneal, variant)
            rep.tooth("t", variant, t, ref, alt)


def check_positions(rep, key, starts, dirs, t, positions, views):
    """K2b on the kernel's own t; ``starts`` / ``dirs``: (R, 3) of the batch's rays (CPU tensors)."""
    check_bits(rep, "positions", key, positions, positions32(starts, dirs, t))
    rep.compare("positions", key, positions, positions64(starts, dirs, t))
    if views is not None:
        check_bits(rep, "views", key, views, dirs.reshape(-1, 1, 3).expand(-1, t.shape[1], 3))


# ------------------------------------------------------------------------------------- K2c
def kernel_depth(n):
    """Sum depth of K2c's running sum: a 64-lane scan and one level per 64-sample row."""
    return WAVE + (n + ROW - 1) // ROW


def _rows_restart(tau):
    """Exclusive product of ``tau`` (R, n) restarted at every 64-sample row (the no_carry tooth)."""
    R, n = tau.shape
    rows = (n + ROW - 1) // ROW
    pad = torch.ones(R, rows * ROW, dtype=tau.dtype, device=tau.device)
    pad[:, :n] = tau
    blk = pad.reshape(R, rows, ROW)
    excl = torch.cat([torch.ones_like(blk[..., :1]), blk[..., :-1]], -1).cumprod(-1)
    return excl.reshape(R, rows * ROW)[:, :n]


def cdf64(t_probe, opacity, logits=False, sum_depth=None, variant=None):
    """V (R, n - 1) of K2c on the f32 probe t (R, n) and sigma (R, n) -- or, with ``logits``, the raw
    (R * n, 4) model outputs whose last column goes through softplus."""
    tt = t_probe.double()
    R, n = tt.shape
    if logits:
        sigma = cr.softplus(opacity.double().reshape(R, n, 4)[..., 3])
    else:
        sigma = V(opacity.double())
    wt = cr.weights(sigma, cr._delta(tt, None))
    # on a certain tie (|sigma delta| < 2^-26, where expf(-x) == 1) the kernel's alpha is exactly 0: its
    # error is the float64 alpha itself, not the 2 ulps of 1 an expf rounding could cost elsewhere
    a = wt["alpha"]
    tie = wt["x"].v.abs() < cr.TIE_SURE
    w = V(a.v, torch.where(tie, a.v.abs() / U, a.b)) * wt["T"]
    if variant == "no_carry":
        T = _rows_restart(wt["tau"].v)
        w = V(wt["alpha"].v * T, w.b)
    lo, hi = dict(cdf_first_weight=(0, n - 2), cdf_last_weight=(2, n)).get(variant, (1, n - 1))
    terms = V(w.v[:, lo:hi], w.b[:, lo:hi])
    v = terms if variant == "no_eps" else terms + EPS5
    depth = kernel_depth(n) if sum_depth is None else sum_depth
    if variant == "no_carry":
        # the running sum restarted at every row, too (the first row's first term is sample 1)
        s = torch.arange(1, n - 1, device=tt.device)
        rv = torch.zeros_like(v.v)
        for r in range((n + ROW - 1) // ROW):
            m = (s // ROW) == r
            rv = rv + torch.where(m[None], torch.where(m[None], v.v, 0.0).cumsum(1), 0.0)
        total = v.v.sum(1, keepdim=True)
        cdf = rv / total
        return V(torch.cat([torch.zeros_like(cdf[:, :1]), cdf], 1), torch.zeros(R, n - 1, dtype=torch.float64,
                                                                                device=tt.device))
    inc = v.v.cumsum(1)
    run_v = inc - v.v if variant == "exclusive_sum" else inc
    run = V(run_v, v.b.cumsum(1) + depth * v.v.abs().cumsum(1) + (n - 2) * TINY)
    total = cr.vsum(v, 1, depth)
    cdf = run / V(total.v[:, None], total.b[:, None])
    zero = torch.zeros_like(cdf.v[:, :1])
    return V(torch.cat([zero, cdf.v], 1), torch.cat([zero, cdf.b], 1))


def check_cdf(rep, key, t_probe, opacity, cdf, logits=False, sum_depth=None, teeth=True):
    """K2c of one batch: invariants, the float64 budget, the teeth."""
    R, n = t_probe.shape
    cdf = cdf.to(t_probe.device)
    if not bool((cdf[:, 0] == 0).all()):
        rep.failures.append("cdf %s: %d rows do not start at 0" % (key, int((cdf[:, 0] != 0).sum())))
    if n > 2 and not bool((cdf[:, -1] == 1.0).all()):
        rep.failures.append("cdf %s: %d rows do not end at 1.0f" % (key, int((cdf[:, -1] != 1.0).sum())))
    down = ~(cdf[:, 1:] >= cdf[:, :-1])
    if bool(down.any()):
        rep.failures.append("cdf %s: %d rows are not non-decreasing (searchsorted needs them to be)"
                            % (key, int(down.any(1).sum())))
    ref = cdf64(t_probe, opacity, logits, sum_depth)
    rep.compare("cdf", key, cdf, ref)
    if teeth:
        for variant in CDF_TEETH:
            rep.tooth("cdf", variant, cdf, ref, cdf64(t_probe, opacity, logits, sum_depth, variant))


# ------------------------------------------------------------------------------------- K2d
def _bins(cdf, u, right=True):
    width = cdf.shape[1]
    k = torch.searchsorted(cdf.contiguous(), u.contiguous(), right=right)
    return (k - 1).clamp_min(0), k.clamp_max(width - 1)


def focus64(near, far, cdf, u, unit, variant=None):
    """V (R, n_focus) of K2d's inverse-transform samples from the f32 near / far (R,), the kernel's own
    CDF rows (R, n_focus - 1), ``u`` (R, n_focus) and ``unit`` (n_focus,), on the kernel's f32 decisions."""
    lo, hi = _bins(cdf, u, variant != "right_false")
    c_lo, c_hi = cdf.gather(1, lo), cdf.gather(1, hi)
    clamp = (c_hi - c_lo) < EPS5                              # (f32, like the kernel)
    if variant == "no_denom_clamp":
        clamp = torch.zeros_like(clamp)
    n, f = V(near.double()[:, None]), V(far.double()[:, None])
    if variant == "annealed_focus":
        n, f = anneal64(n, f, FOCUS_ANNEAL)
    span = f - n
    un = unit.double().to(near.device)

    def grid(j):
        return n + V(un[j]) * span

    if variant == "bin_edges":
        t_lo, t_hi = grid(lo), grid(hi)
    else:
        t_lo, t_hi = (grid(lo) + grid(lo + 1)) * 0.5, (grid(hi) + grid(hi + 1)) * 0.5
    sub = V(c_hi.double()) - c_lo.double()
    denom = V(torch.where(clamp, 1.0, sub.v), torch.where(clamp, 0.0, sub.b))
    frac = (V(u.double()) - c_lo.double()) / denom
    return t_lo + frac * (t_hi - t_lo)


def focus32(near, far, cdf, u, unit):
    """The oracle's f32 sequence (CPU tensors)."""
    return orc.focus_t(near, far, cdf, u, unit)


def check_merge(rep, key, near, far, cdf, u, unit, uniform_in, row, teeth=True):
    """K2d of one batch (CPU tensors): ``near`` / ``far`` (R,) of the batch's rays, their CDF rows, the
    uniform half the kernel was given, the row it wrote."""
    focus = focus32(near, far, cdf, u, unit)
    want = torch.sort(torch.cat([uniform_in, focus], 1), 1).values
    check_bits(rep, "row", key, row, want)
    ref = focus64(near, far, cdf, u, unit)
    rep.compare("focus", key, focus, ref)
    if teeth:
        for variant in MERGE_TEETH:
            rep.tooth("focus", variant, focus, ref, focus64(near, far, cdf, u, unit, variant))


# ------------------------------------------------------------------------------------- data
CDF_REGIMES = ("empty", "opaque_first", "opaque_interior", "spike", "bumps", "tie_windows", "repeated_t",
               "logit_20", "logit_extremes")


def probe_t(R, n, seed, near=None, far=None):
    """(R, n) f32 probe t = linspace(near, far, n) per ray, near in [0.1, 2], far - near in [0.5, 4]."""
    g = torch.Generator().manual_seed(seed)
    if near is None:
        near = (0.1 + 1.9 * torch.rand(R, generator=g)).float()
        far = (near.double() + 0.5 + 3.5 * torch.rand(R, generator=g, dtype=torch.float64)).float()
    unit = torch.linspace(0, 1, n)
    return orc.linspace_rows(near, far, n, unit), near, far


def make_probe(R, n, seed):
    """(t (R, n), logits (R * n, 4), sigma (R, n)) f32; ray r is in regime
    ``CDF_REGIMES[(r + seed) % len(CDF_REGIMES)]``:

    * empty: sigma logits in [-40, -20] (sigma delta far below 2^-26);
    * opaque_first: sample 0 opaque (sigma delta ~ 30), the rest thin;
    * opaque_interior: one inner sample opaque, the rest empty: the CDF is flat (steps of ~1e-5)
      around one jump, where the denom clamp decides;
    * spike: one inner sample with sigma delta ~ 1, the rest thin;
    * bumps: two smooth bumps of density;
    * tie_windows: sigma delta across 2^-26 .. 2^-22 (the tau = 1 clamp windows);
    * repeated_t: t in equal pairs (delta = 0);
    * logit_20: sigma logits at 20 and one ulp either side;
    * logit_extremes: sigma logits at -100 and at 1e4.

    ``sigma`` is softplus(logits) (the plain K2c form gets the same densities)."""
    g = torch.Generator().manual_seed(seed)

    def rnd(*shape):
        return torch.rand(*shape, generator=g, dtype=torch.float64)

    t, near, far = probe_t(R, n, seed)
    regime = (torch.arange(R) + seed) % len(CDF_REGIMES)
    is_ = {name: (regime == i)[:, None] for i, name in enumerate(CDF_REGIMES)}
    td = t.clone()
    td[:, 1::2] = t[:, 0:n - 1:2][:, :td[:, 1::2].shape[1]]
    t = torch.where(is_["repeated_t"], td, t)
    tt = t.double()
    delta = torch.cat([tt[:, 1:] - tt[:, :-1], tt[:, -1:] - tt[:, -2:-1]], 1).clamp_min(1e-3)
    s = torch.arange(n, dtype=torch.float64)[None]
    inv = cr._inv_softplus
    lg = torch.randn(R, n, 4, generator=g, dtype=torch.float64) * 2.0
    w = lg[..., 3].clone()
    w = torch.where(is_["empty"], -20.0 - 20.0 * rnd(R, n), w)
    thin = inv(0.01 * rnd(R, n) / delta)
    first = torch.where(s == 0, inv(30.0 / delta), thin)
    w = torch.where(is_["opaque_first"], first, w)
    j = 1 + (rnd(R, 1) * (n - 2)).long().clamp_max(n - 3).double()
    w = torch.where(is_["opaque_interior"], torch.where(s == j, inv(30.0 / delta), -40.0 - 10.0 * rnd(R, n)), w)
    w = torch.where(is_["spike"], torch.where(s == j, inv((0.5 + rnd(R, 1)) / delta), thin), w)
    c1, c2 = rnd(R, 1) * n, rnd(R, 1) * n
    bump = 3.0 * torch.exp(-((s - c1) / (0.1 * n + 1)) ** 2) + 1.5 * torch.exp(-((s - c2) / (0.05 * n + 1)) ** 2)
    w = torch.where(is_["bumps"], inv(bump / delta + 1e-6), w)
    x = 2.0 ** (-27.0 + 6.0 * rnd(R, n))                      # sigma delta in 2^-27 .. 2^-21
    w = torch.where(is_["tie_windows"], inv(x / delta), w)
    up = float(np.nextafter(np.float32(20.0), np.float32(np.inf)))
    down = float(np.nextafter(np.float32(20.0), np.float32(-np.inf)))
    pick = rnd(R, n)
    w = torch.where(is_["logit_20"], torch.where(pick < 1 / 3, 20.0, torch.where(pick < 2 / 3, up, down)), w)
    w = torch.where(is_["logit_extremes"], torch.where(pick < 0.5, -100.0, 1e4), w)
    lg[..., 3] = w
    logits = lg.float()
    sigma = torch.nn.functional.softplus(logits[..., 3])
    return t.contiguous(), logits.reshape(R * n, 4).contiguous(), sigma.contiguous()


def make_u(cdf, n_focus, seed, mode):
    """(R, n_focus) f32 uniforms: ``linspace`` (0 and 1 included), ``rand``, ``entries`` (every other
    value an entry of the ray's own CDF row, the rest rand) or ``top`` (nextafter(1, 0) and 1)."""
    R = cdf.shape[0]
    g = torch.Generator().manual_seed(seed)
    if mode == "linspace":
        return torch.linspace(0, 1, n_focus).repeat(R, 1).contiguous()
    u = torch.rand(R, n_focus, generator=g)
    if mode == "entries":
        j = torch.randint(0, cdf.shape[1], (R, n_focus), generator=g)
        u = torch.where(torch.arange(n_focus)[None] % 2 == 0, cdf.gather(1, j), u)
    elif mode == "top":
        below = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
        u[:, 0::2] = below
        u[:, 1::2] = 1.0
    return u.contiguous()
