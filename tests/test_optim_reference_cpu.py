"""The K7 checker (tests/optim_reference.py) on its own float32 restatement of the kernel, no GPU
needed: the restatement must sit inside the float64 budget on the cases of
tests/test_optim_reference_gpu.py, every deliberately changed reference must fail on it, one flipped
ulp must fail the bit-exact check, and one value off by more than its budget the float64 check."""

import math

import numpy as np
import pytest
import torch

from tests import optim_reference as orf

SIZES = [1, 255, 256, 257, 1023, 1024, 1025, 262144, 262145, 263428]


def _run(p, g, m, v, a, fixed=True):
    e = orf.emulate(p.numpy(), g.numpy(), m.numpy(), v.numpy(), a, fixed=fixed)
    return {k: torch.from_numpy(e[k]) for k in orf.OUTS}, e


def _case(n, regime, caller, step, seed):
    g = orf.make_grads(n, regime, seed)
    p, m, v = orf.make_state(n, step, seed)
    return p, g, m, v, orf.kernel_args(step, 5e-4, **orf.CALLERS[caller])


@pytest.mark.parametrize("n", SIZES)
def test_restatement_inside_the_budget_and_teeth_fire(n):
    rep = orf.new_report()
    i = 0
    for regime in orf.REGIMES:
        for caller in orf.CALLERS:
            step = orf.STEPS[i % len(orf.STEPS)]
            i += 1
            p, g, m, v, a = _case(n, regime, caller, step, 1000 * n + i)
            out, want = _run(p, g, m, v, a)
            orf.check_bits(rep, "n=%d" % n, out, want)
            orf.check(rep, "n=%d %s %s step %d" % (n, regime, caller, step), p, g, m, v, a, out)
    problems = rep.problems(orf.TEETH)
    assert not problems, "\n".join(problems)
    for out, worst in rep.worst.items():
        assert worst <= orf.KAPPA[out], (out, worst)


def test_regimes_do_what_they_say():
    n = 4099
    norms = {}
    for regime in orf.REGIMES:
        p, g, m, v, a = _case(n, regime, "train", 2, 3)
        gc = g.double().clamp(-orf.f32(0.1), orf.f32(0.1))
        norms[regime] = float(gc.norm())
        if regime == "value_clip":
            assert float((g.abs() > 0.1).double().mean()) > 0.2
        if regime == "at_clip":
            assert float((gc.abs() == orf.f32(0.1)).double().mean()) == 1.0
    assert norms["norm_clip"] > 0.25 and norms["no_clip"] < 0.05 and norms["zero"] == 0.0
    assert abs(norms["window"] - (0.1 - orf.EPS_NORM)) < 1e-7


def test_norm_depth_counts_the_partials_per_thread():
    assert orf.norm_depth(1) == 4 + 6 + 2 + 1 + 6 + 2
    assert orf.norm_depth(262144) == orf.norm_depth(1)              # 256 partials: one per thread
    assert orf.norm_depth(262145) == orf.norm_depth(1) + 1
    assert orf.norm_depth(4 * 128 ** 3 + 4) == orf.norm_depth(1) + 32   # 8193 partials: 33 for thread 0


@pytest.mark.parametrize("n,caller,regimes", [(1025, "train", ("value_clip", "norm_clip", "no_clip", "window")),
                                              (263428, "train_wd", ("norm_clip", "value_clip", "at_clip", "zero")),
                                              (262145, "regression", ("no_clip", "value_clip", "zero", "norm_clip"))])
def test_restatement_trajectory_inside_the_budget(n, caller, regimes):
    """The GPU file's trajectories, each step from the state the restatement's previous step left."""
    rep = orf.new_report()
    p, _, m, v, _ = _case(n, "zero", caller, 1, 5)
    for step in range(1, 7):
        g = orf.make_grads(n, regimes[step % len(regimes)], 31 * step + n)
        a = orf.kernel_args(step, 5e-4 * 0.9 ** step, **orf.CALLERS[caller])
        out, _ = _run(p, g, m, v, a)
        orf.check(rep, "trajectory %s step %d" % (caller, step), p, g, m, v, a, out, teeth=False)
        p, m, v = out["p"], out["m"], out["v"]
    assert not rep.failures, "\n".join(rep.failures)
    for out, worst in rep.worst.items():
        assert worst <= orf.KAPPA[out], (out, worst)


@pytest.mark.parametrize("n", [1, 1025, 262145])
def test_overflowing_norm_with_infinite_bounds(n):
    """+inf bounds, f32 sum of squares beyond the range: the fixed kernel's step is unclipped Adam and
    within the budget; the kernel before the fix (inf / inf = NaN as coefficient) is all NaN."""
    g = (torch.randn(n, generator=torch.Generator().manual_seed(n)) * 1e20).float()
    g[0] = 2e20
    p, m, v = orf.make_state(n, 3, n)
    a = orf.kernel_args(3, 5e-4, **orf.CALLERS["regression"])
    out, _ = _run(p, g, m, v, a)
    assert float(out["norm"]) == math.inf and bool(torch.isfinite(out["p"]).all())
    rep = orf.new_report()
    orf.check(rep, "overflow", p, g, m, v, a, out, teeth=False)
    assert not rep.failures, "\n".join(rep.failures)
    old, _ = _run(p, g, m, v, a, fixed=False)
    assert bool(torch.isnan(old["p"]).all())
    rep = orf.new_report()
    orf.check(rep, "overflow, unfixed", p, g, m, v, a, old, teeth=False)
    assert rep.failures


def test_fix_keeps_every_other_bit():
    """The +inf special case changes nothing where the norm is finite (max_norm finite or not)."""
    for caller in orf.CALLERS:
        p, g, m, v, a = _case(3000, "norm_clip", caller, 10, 5)
        new, _ = _run(p, g, m, v, a)
        old, _ = _run(p, g, m, v, a, fixed=False)
        for o in orf.OUTS:
            assert torch.equal(new[o].view(torch.int32), old[o].view(torch.int32)), (caller, o)


def test_one_flipped_ulp_fails_the_bit_check():
    p, g, m, v, a = _case(1025, "norm_clip", "train_wd", 10, 2)
    out, want = _run(p, g, m, v, a)
    rep = orf.new_report()
    orf.check_bits(rep, "clean", out, want)
    assert not rep.failures
    bad = dict(out, p=out["p"].clone())
    bad["p"][700] = float(np.nextafter(np.float32(bad["p"][700]), np.float32(np.inf)))
    orf.check_bits(rep, "flipped", bad, want)
    assert len(rep.failures) == 1 and rep.failures[0].startswith("p flipped: 1 of 1025")


@pytest.mark.parametrize("o", orf.OUTS)
def test_one_value_beyond_its_budget_fails(o):
    p, g, m, v, a = _case(1025, "norm_clip", "train_wd", 10, 2)
    out, _ = _run(p, g, m, v, a)
    ref = orf.reference(p, g, m, v, a)
    i = 0 if o == "norm" else 513
    bad = dict(out, **{o: out[o].clone()})
    off = 3.0 * orf.KAPPA[o] * orf.U * float(ref[o].b[i])
    bad[o][i] = float(ref[o].v[i] + off)
    rep = orf.new_report()
    orf.check(rep, "off", p, g, m, v, a, bad, teeth=False)
    assert len(rep.failures) == 1 and rep.failures[0].startswith(o + " off: 1 of"), rep.failures
