"""Float64 reference of K7, the clip + Adam kernel pair (csrc/optim.hip), with a first-order error
budget for every output element, and a float32 restatement of the kernel that must match it bit for bit.

K7 is ``clip_grad_value_`` -> ``clip_grad_norm_`` -> Adam with coupled (L2) weight decay over one flat
f32 buffer of n parameters (ray_caster.py / the regression loops):

* launch 1, one workgroup of 256 threads per 1024 elements: clamp by value, write the clamped
  gradient, and the workgroup's sum of squares into ``partial[block]``;
* launch 2, the same grid: every workgroup re-reduces all ``P = ceil(n / 1024)`` partials in the same
  fixed order, ``norm = sqrtf(total)``, ``coef = min(1, max_norm / (norm + 1e-6f))``, then
  ``g = grad coef`` (written back), ``g += wd p`` (skipped when ``wd == 0``),
  ``m += (g - m)(1 - b1)``, ``v = v b2 + ((1 - b2) g) g``, ``p -= step_size (m / (sqrt(v) isb2 + eps))``.
  Workgroup 0, thread 0 writes ``norm`` to ``grad_norm_out``.

The arguments are the kernel's own f32 values (``kernel_args``): ``ops.clip_adam`` computes
``step_size = lr / (1 - b1^step)`` and ``isb2 = 1 / sqrt(1 - b2^step)`` in double and rounds them to
f32; ``1 - b1`` and ``1 - b2`` are exact in f32 for the betas used here (Sterbenz).

**Float64 budgets** (``reference``) are carried by ``composite_reference.V``.  The sum of squares is a
sum of non-negative terms on a tree of depth ``norm_depth(n)``: up to four products per thread, the
6-level wave butterfly, the ``(r0 + r1) + (r2 + r3)`` pair, ``ceil(P / 256)`` partials per thread in the
second launch, then the butterfly and the pair again.  The min(1, .) follows the kernel's f32 decision:
where the budget of ``max_norm / (norm + 1e-6)`` reaches 1 either branch is accepted, and the one the
kernel took is read from its written gradients.  A sum of squares beyond the f32 range is the kernel's
``inf`` (exact); with ``max_norm = +inf`` the coefficient is exactly 1 whatever the norm.

**Bit-exact f32** (``emulate``): optim.hip is compiled with ``-ffp-contract=off`` and IEEE ``sqrtf`` /
division, the reduction order is fixed, and lane 0 of a wave64 ``__shfl_xor`` butterfly sums the pairs
``(i, i + 32)``, then ``(i, i + 16)``, ...  So numpy float32 op by op reproduces every output.

Teeth (``TEETH``): the reference is recomputed with one deliberate change each; the kernel's output must
fail every one, and each must touch the data and exceed the bound somewhere (``Report.problems``).
"""

import math

import numpy as np
import torch

from tests import composite_reference as cr
from tests.composite_reference import TINY, U, V, WAVE

F32_MAX = float(np.finfo(np.float32).max)
EPS_NORM = float(np.float32(1e-6))
PAIR = 2                     # levels of the (r0 + r1) + (r2 + r3) pair of block_sum_256
PER_THREAD = 4               # gradient elements per thread in launch 1

# kappa per output, fixed.  Measured on an MI355X over every case of tests/test_optim_reference_gpu.py
# (K7 is f32 in every arithmetic mode) and set to about twice the worst ratio |err| / (2^-24 budget)
# seen, which is given after each value.
KAPPA = dict(grads=0.4,          # [0.171]
             norm=0.3,           # [0.125]
             m=2.0,              # [0.982]
             v=2.0,              # [0.997]
             p=2.0)              # [0.998]

TEETH = ("unclamped_norm", "coef_unclamped", "no_eps_norm", "no_bc1", "no_bc2", "eps_in_sqrt", "adamw",
         "decay_before_clip", "mv_unclipped", "tail_partial_missing")
TEETH_DOC = dict(unclamped_norm="the norm taken over the gradients before the clamp by value",
                 coef_unclamped="coef = max_norm / (norm + 1e-6) not clamped to 1",
                 no_eps_norm="coef = max_norm / norm (the 1e-6 dropped)",
                 no_bc1="step_size = lr (bias correction 1 dropped)",
                 no_bc2="v not bias-corrected (isb2 = 1)",
                 eps_in_sqrt="denominator sqrt(v / bc2 + eps) instead of sqrt(v / bc2) + eps",
                 adamw="decoupled decay p (1 - lr wd) instead of the L2 term in the gradient",
                 decay_before_clip="wd p added to the gradient before the norm clip",
                 mv_unclipped="m and v fed the gradient before either clip",
                 tail_partial_missing="the last workgroup's partial missing from the norm")
OUTS = ("grads", "norm", "m", "v", "p")
NORM_TEETH = ("unclamped_norm", "no_eps_norm", "decay_before_clip", "tail_partial_missing")   # (change coef)


def new_report():
    return cr.Report(KAPPA, TEETH_DOC)


def f32(x):
    return float(np.float32(x))


def blocks_of(n):
    return (n + 1023) // 1024


def norm_depth(n):
    """Depth of the kernel's sum-of-squares tree over n elements (module docstring)."""
    P = blocks_of(n)
    return PER_THREAD + WAVE + PAIR + -(-P // 256) + WAVE + PAIR


def kernel_args(step, lr, weight_decay=0.0, clip_value=0.1, max_norm=0.1, beta1=0.9, beta2=0.999, eps=1e-8):
    """The f32 scalars ``ops.clip_adam`` hands K7 (as Python floats), and the caller's lr / step."""
    return dict(clip_value=f32(clip_value), max_norm=f32(max_norm),
                step_size=f32(lr / (1.0 - beta1 ** step)), inv_sqrt_bc2=f32(1.0 / math.sqrt(1.0 - beta2 ** step)),
                beta1=f32(beta1), beta2=f32(beta2), eps=f32(eps), weight_decay=f32(weight_decay),
                lr=float(lr), step=int(step), beta1_64=float(beta1), beta2_64=float(beta2))


# ------------------------------------------------------------------------------------- bit-exact f32
def _lane0_butterfly(x):
    """Lane 0 of the wave64 __shfl_xor butterfly over the last axis (64 lanes)."""
    while x.shape[-1] > 1:
        h = x.shape[-1] // 2
        x = x[..., :h] + x[..., h:]
    return x[..., 0]


def _block_sum_256(x):
    """block_sum_256 of (..., 256) float32: the four wave totals paired (r0 + r1) + (r2 + r3)."""
    r = _lane0_butterfly(x.reshape(x.shape[:-1] + (4, 64)))
    return (r[..., 0] + r[..., 1]) + (r[..., 2] + r[..., 3])


def emulate(p, g, m, v, a, fixed=True):
    """K7 in numpy float32, op by op.  ``p, g, m, v``: float32 arrays (not modified); ``a``: kernel_args.
    ``fixed=False`` is the kernel before the ``max_norm = +inf`` fix.
    Returns dict(grads, norm, m, v, p, partial) of float32 arrays."""
    f = np.float32
    p, g, m, v = (np.asarray(x, dtype=np.float32) for x in (p, g, m, v))
    n = g.size
    P = blocks_of(n)
    with np.errstate(all="ignore"):
        cv = f(a["clip_value"])
        gc = np.where(g < -cv, -cv, np.where(g > cv, cv, g)).astype(np.float32)
        sq = np.zeros(P * 1024, dtype=np.float32)
        sq[:n] = gc * gc
        sq = sq.reshape(P, PER_THREAD, 256)
        acc = sq[:, 0]
        for k in range(1, PER_THREAD):
            acc = acc + sq[:, k]
        partial = _block_sum_256(acc)
        J = -(-P // 256)
        pp = np.zeros(J * 256, dtype=np.float32)
        pp[:P] = partial
        pp = pp.reshape(J, 256)
        acc = pp[0]
        for j in range(1, J):
            acc = acc + pp[j]
        norm = np.sqrt(_block_sum_256(acc))
        max_norm = f(a["max_norm"])
        if fixed and np.isinf(max_norm) and max_norm > 0:
            coef = f(1.0)
        else:
            coef = max_norm / (norm + f(EPS_NORM))
            coef = f(1.0) if coef > f(1.0) else coef
        gs = gc * coef
        wd = f(a["weight_decay"])
        ge = gs + wd * p if wd != f(0.0) else gs
        b1, b2 = f(a["beta1"]), f(a["beta2"])
        mi = m + (ge - m) * (f(1.0) - b1)
        vi = v * b2 + ((f(1.0) - b2) * ge) * ge
        denom = np.sqrt(vi) * f(a["inv_sqrt_bc2"]) + f(a["eps"])
        pn = p - f(a["step_size"]) * (mi / denom)
    return dict(grads=gs, norm=np.array([norm], dtype=np.float32), m=mi, v=vi, p=pn, partial=partial)


# ------------------------------------------------------------------------------------- float64
def _sqrt(x):
    """sqrt with one rounding; the first-order term capped by sqrt(|delta|) (valid at 0)."""
    y = x.v.sqrt()
    first = x.b / (2.0 * y)
    cap = (x.b * U).sqrt() / U
    b = torch.where(y > 0, torch.minimum(first, cap), cap)
    return V(y, b + y + TINY)


def _const(x, like):
    return V(torch.full_like(like, x))


def _sumsq(gc, tail_missing=False):
    """(value, budget) of the kernel's f32 sum of squares of the clamped gradients gc (float64 tensor)."""
    n = gc.numel()
    sq = gc * gc
    if tail_missing:
        sq = sq[:(blocks_of(n) - 1) * 1024]
    S = float(sq.sum())
    return S, S * (1 + norm_depth(n)) + n * TINY


def _norm_of(S, bS, device):
    """V of sqrtf(sum): inf (exact) beyond the f32 range, an error where it cannot be decided."""
    lo, hi = S - bS * U * 4, S + bS * U * 4
    if lo > F32_MAX:
        return V(torch.tensor([math.inf], dtype=torch.float64, device=device),
                 torch.zeros(1, dtype=torch.float64, device=device))
    if hi > F32_MAX:
        raise ValueError("the sum of squares %r lies within its budget of the f32 overflow" % S)
    return _sqrt(V(torch.tensor([S], dtype=torch.float64, device=device),
                   torch.tensor([bS], dtype=torch.float64, device=device)))


def coef_of(norm, a, variant=None):
    """V of max_norm / (norm + 1e-6) before the min(1, .); None for max_norm = +inf (coef exactly 1)."""
    max_norm = a["max_norm"]
    if math.isinf(max_norm) and max_norm > 0:
        return None
    if variant == "no_eps_norm":
        return max_norm / norm
    return max_norm / (norm + EPS_NORM)


def reference(p, g, m, v, a, variant=None, branch=None):
    """dict of V (float64 on the CPU) for grads, norm, m, v, p.  ``p, g, m, v``: float32 tensors;
    ``branch``: ``"one"`` / ``"coef"``, the min(1, .) branch where the budget allows both (see
    ``decide``)."""
    p, g, m, v = (x.detach().double().reshape(-1) for x in (p, g, m, v))
    cv = a["clip_value"]
    gc = g.clamp(-cv, cv) if not math.isinf(cv) else g.clone()
    wd = a["weight_decay"]
    norm_src = g if variant == "unclamped_norm" else gc
    if variant == "decay_before_clip" and wd != 0.0:
        norm_src = norm_src + wd * p
    S, bS = _sumsq(norm_src, tail_missing=variant == "tail_partial_missing")
    norm = _norm_of(S, bS, p.device)
    cf = coef_of(norm, a, variant)
    one = V(torch.ones(1, dtype=torch.float64, device=p.device), torch.zeros(1, dtype=torch.float64, device=p.device))
    if cf is None:
        coef = one
    else:
        if variant == "coef_unclamped":
            take_one = False
        elif branch is not None and variant not in NORM_TEETH:
            take_one = branch == "one"
        else:
            take_one = bool(cf.v[0] > 1.0) or bool(torch.isnan(cf.v[0]))
        coef = one if take_one else cf
    if variant == "decay_before_clip" and wd != 0.0:
        src = V(gc + wd * p)            # (the kernel's own clip of the decayed gradient, first order)
        gs = src * coef
        ge = gs
    else:
        gs = V(gc).exact_mul(coef) if bool(coef.v[0] == 1.0) and bool(coef.b[0] == 0) else V(gc) * coef
        ge = gs
        if variant == "mv_unclipped":
            ge = V(g)
        if wd != 0.0 and variant != "adamw":
            ge = ge + V(p) * wd
    c1 = 1.0 - a["beta1"]
    c2 = 1.0 - a["beta2"]
    M, Vv, P = V(m), V(v), V(p)
    mi = M + (ge - M) * c1
    vi = Vv * a["beta2"] + (ge * c2) * ge
    isb = 1.0 if variant == "no_bc2" else a["inv_sqrt_bc2"]
    if variant == "eps_in_sqrt":
        denom = _sqrt(vi * (isb * isb) + a["eps"])
    else:
        denom = _sqrt(vi) * isb + a["eps"]
    step_size = f32(a["lr"]) if variant == "no_bc1" else a["step_size"]
    pn = P - (mi / denom) * step_size
    if variant == "adamw" and wd != 0.0:
        pn = (P - P * (a["lr"] * wd)) - (mi / denom) * step_size
    return dict(grads=gs, norm=norm, m=mi, v=vi, p=pn)


def decide(p, g, m, v, a, grads_out):
    """The min(1, .) branch: ``None`` where the budget decides it, else the one the kernel took, read from
    its written gradients (equal to the clamped gradients everywhere: "one")."""
    g64 = g.detach().double().reshape(-1)
    cv = a["clip_value"]
    gc = g64.clamp(-cv, cv) if not math.isinf(cv) else g64
    norm = _norm_of(*_sumsq(gc), g64.device)
    cf = coef_of(norm, a)
    if cf is None or torch.isnan(cf.v[0]):
        return None
    reach = KAPPA["norm"] * U * float(cf.b[0]) * 4
    if abs(float(cf.v[0]) - 1.0) > reach:
        return None
    same = torch.equal(grads_out.detach().reshape(-1).to(gc.device), gc.float())
    return "one" if same else "coef"


def check(rep, key, p, g, m, v, a, out, teeth=True):
    """Compares K7's outputs ``out`` (dict grads, norm, m, v, p of tensors) with the float64 reference of
    the inputs ``p, g, m, v`` (the buffers before the launch) and records the teeth."""
    branch = decide(p, g, m, v, a, out["grads"])
    ref = reference(p, g, m, v, a, branch=branch)
    for o in OUTS:
        _compare(rep, o, key, out[o], ref[o])
    if not teeth:
        return
    for name in TEETH:
        alt = reference(p, g, m, v, a, variant=name)
        for o in OUTS:
            got, r, al = out[o].detach().double().reshape(-1).to(ref[o].v.device), ref[o], alt[o]
            fin = torch.isfinite(r.v) & torch.isfinite(al.v)
            touched_nonfinite = bool((torch.isfinite(r.v) != torch.isfinite(al.v)).any())
            if touched_nonfinite:
                far = float("inf") if bool((torch.isfinite(got) != torch.isfinite(al.v)).any()) else 0.0
                t = rep.teeth.setdefault(name, dict(touched=True, exceeds=False, ratio=0.0, out=None))
                t["exceeds"] = True
                if far > t["ratio"]:
                    t["ratio"], t["out"] = far, o
            rep.tooth(o, name, got[fin], V(r.v[fin], r.b[fin]), V(al.v[fin], al.b[fin]))


def _compare(rep, out, key, got, ref):
    """Finite reference elements against the budget; non-finite ones (the norm's inf) exactly."""
    got = got.detach().double().reshape(-1).to(ref.v.device)
    fin = torch.isfinite(ref.v)
    rep.compare(out, key, got[fin], V(ref.v[fin], ref.b[fin]))
    g, r = got[~fin], ref.v[~fin]
    same = (g == r) | (torch.isnan(g) & torch.isnan(r))
    if not bool(same.all()):
        rep.failures.append("%s %s: %d non-finite reference elements differ" % (out, key, int((~same).sum())))


def check_bits(rep, key, out, want):
    """Every output of the kernel equal, bit for bit, to ``emulate``'s."""
    for o in OUTS:
        got = out[o].detach().cpu().reshape(-1).contiguous().view(torch.int32)
        w = torch.from_numpy(np.ascontiguousarray(want[o]).reshape(-1)).view(torch.int32)
        diff = got != w
        if bool(diff.any()):
            i = int(diff.nonzero()[0, 0])
            rep.failures.append("%s %s: %d of %d elements differ from the f32 restatement in their bits, first at "
                                "flat index %d: got %r want %r" % (o, key, int(diff.sum()), diff.numel(), i,
                                                                   float(got[i:i + 1].view(torch.float32)),
                                                                   float(w[i:i + 1].view(torch.float32))))


# ------------------------------------------------------------------------------------- cases
CALLERS = dict(train=dict(clip_value=0.1, max_norm=0.1, weight_decay=0.0),
               train_wd=dict(clip_value=0.1, max_norm=0.1, weight_decay=1e-3),
               regression=dict(clip_value=math.inf, max_norm=math.inf, weight_decay=1e-3,
                               beta1=0.9, beta2=0.999, eps=1e-8))
REGIMES = ("value_clip", "norm_clip", "no_clip", "window", "zero", "at_clip")
STEPS = (1, 2, 10, 10000)


def make_grads(n, regime, seed, max_norm=0.1, clip_value=0.1):
    """float32 (n,) gradients of one regime (for the 0.1 / 0.1 bounds of TrainEngine):

    value_clip: about a third beyond +-clip_value; norm_clip: inside the clamp, norm about 3x max_norm;
    no_clip: norm about max_norm / 3; window: norm within a few ulps of max_norm - 1e-6 (coef ~ 1);
    zero: all 0; at_clip: every element exactly +-clip_value, a few just beyond."""
    gen = torch.Generator().manual_seed(seed)
    if regime == "zero":
        return torch.zeros(n)
    if regime == "at_clip":
        s = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)
        g = (s * f32(clip_value)).float()
        k = max(1, n // 7)
        g[:k] = g[:k] * 1.5
        return g
    x = torch.randn(n, generator=gen, dtype=torch.float64)
    if regime == "value_clip":
        return (x * clip_value * 1.1).float()
    x = x.clamp(-3, 3)
    want = dict(norm_clip=3.0 * max_norm, no_clip=max_norm / 3.0, window=max_norm - EPS_NORM)[regime]
    g = (x * (want / float(x.norm()))).float()
    if regime == "window":
        # nudge the largest element until the f32 norm sits on max_norm - 1e-6
        g32 = g.double()
        gc = g32.clamp(-clip_value, clip_value)
        err = want - float(gc.norm())
        i = int(gc.abs().argmax())
        g[i] = float(g[i]) + err * float(gc.norm()) / float(g[i])
    return g


def make_state(n, step, seed, p_scale=0.05):
    """(p, m, v) float32: m = v = 0 at step 1, random m and v >= 0 otherwise."""
    gen = torch.Generator().manual_seed(seed + 7)
    p = (torch.randn(n, generator=gen) * p_scale).float()
    if step == 1:
        return p, torch.zeros(n), torch.zeros(n)
    m = (torch.randn(n, generator=gen) * 0.01).float()
    v = (torch.rand(n, generator=gen) ** 2 * 1e-4).float()
    return p, m, v
