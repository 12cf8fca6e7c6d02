"""K7 (clip + Adam, csrc/optim.hip) against float64 with error budgets and against its float32
restatement bit for bit (tests/optim_reference.py).

Every launch goes through ``ops.clip_adam`` with ``scratch`` (longer than the P partials) and the norm
output filled with NaN.  Sizes cover the tails of n against 256 and 1024, exactly 256 partials, the tiny
NeRF and the voxel engine (8193 partials: thread 0 of the re-reduction adds 33, the others 32); states
``m = v = 0`` at step 1 and random moments at steps 2, 10 and 10 000; the bounds of TrainEngine (0.1 /
0.1, wd 0 and 1e-3) and of RegressionEngine (+inf / +inf, wd 1e-3); gradients clipped by value, by the
norm, not at all, with the norm on max_norm - 1e-6, all zero and exactly at +-clip_value.  Three
trajectories run several steps on the kernel's own state; a real TrainEngine and RegressionEngine step
are checked from a snapshot of K7's inputs.  K7 is f32 in every arithmetic mode, so the file runs
unchanged under ``--precision bf16x6``."""

import json

import pytest
import torch

from fourier_feature_nets_amd import ops
from tests import optim_reference as orf

pytestmark = pytest.mark.gpu

SIZES = [1, 255, 256, 257, 1023, 1024, 1025, 262144, 262145, 263428]
VOXEL_N = 4 * 128 ** 3 + 4          # 8193 partials
LR = 5e-4


def dev():
    return torch.device("cuda:0")


def _report(rep, what, **kw):
    teeth = {k: (float("%.3g" % v["ratio"]), v["out"]) for k, v in rep.teeth.items()}
    print("optim reference", json.dumps(dict(what=what, worst=rep.worst, teeth=teeth, **kw)))


def _launch(p, g, m, v, step, caller, lr=LR):
    """One ops.clip_adam on copies of (p, g, m, v) (device tensors); returns the outputs and the partials."""
    n = p.numel()
    P = orf.blocks_of(n)
    kw = dict(orf.CALLERS[caller])
    scratch = torch.full((P + 67,), float("nan"), device=dev())
    norm = torch.full((1,), float("nan"), device=dev())
    p, g, m, v = (x.clone() for x in (p, g, m, v))
    ops.clip_adam(p, g, m, v, step, lr, scratch=scratch, norm_out=norm, **kw)
    torch.cuda.synchronize()
    assert bool(torch.isnan(scratch[P:]).all()), "K7 wrote past the %d partials of its scratch" % P
    return dict(grads=g, norm=norm, m=m, v=v, p=p), scratch[:P]


def _check(rep, key, p, g, m, v, step, caller, out, partial, teeth=True, lr=LR):
    a = orf.kernel_args(step, lr, **orf.CALLERS[caller])
    want = orf.emulate(p.cpu().numpy(), g.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy(), a)
    orf.check_bits(rep, key, out, want)
    if not torch.equal(partial.cpu().view(torch.int32), torch.from_numpy(want["partial"]).view(torch.int32)):
        rep.failures.append("partials %s differ from the f32 restatement" % key)
    orf.check(rep, key, p, g, m, v, a, out, teeth=teeth)


def _case(n, regime, caller, step, seed):
    g = orf.make_grads(n, regime, seed)
    p, m, v = orf.make_state(n, step, seed)
    return tuple(x.to(dev()) for x in (p, g, m, v))


def _problems(rep, required=orf.TEETH):
    p = rep.problems(required)
    for out, worst in rep.worst.items():
        if worst > orf.KAPPA[out]:
            p.append("%s: worst ratio %.3g above kappa" % (out, worst))
    return p


@pytest.mark.parametrize("n", SIZES)
def test_clip_adam_sizes_states_regimes(n):
    rep = orf.new_report()
    i = 0
    for regime in orf.REGIMES:
        for caller in orf.CALLERS:
            step = orf.STEPS[i % len(orf.STEPS)]
            i += 1
            p, g, m, v = _case(n, regime, caller, step, 1000 * n + i)
            out, partial = _launch(p, g, m, v, step, caller)
            _check(rep, "n=%d %s %s step %d" % (n, regime, caller, step), p, g, m, v, step, caller, out, partial)
    _report(rep, "n=%d" % n)
    problems = _problems(rep)
    assert not problems, "\n".join(problems)


@pytest.mark.parametrize("caller,regime,step", [("train", "value_clip", 2), ("train_wd", "norm_clip", 10),
                                                ("regression", "no_clip", 10000)])
def test_clip_adam_voxel_engine_size(caller, regime, step):
    """4 * 128^3 + 4 parameters: 8193 partials, so thread 0 of the re-reduction adds 33 of them.  The
    last workgroup's four gradients carry a good part of the norm, so a missing 33rd partial shows."""
    rep = orf.new_report()
    p, g, m, v = _case(VOXEL_N, regime, caller, step, 77)
    g[:-4] *= 1e-3
    g[-4:] = torch.tensor([0.1, -0.1, 0.05, -0.07])
    out, partial = _launch(p, g, m, v, step, caller)
    _check(rep, "voxels %s %s" % (caller, regime), p, g, m, v, step, caller, out, partial, teeth=False)
    a = orf.kernel_args(step, LR, **orf.CALLERS[caller])
    ref = orf.reference(p, g, m, v, a)
    alt = orf.reference(p, g, m, v, a, variant="tail_partial_missing")
    rep.tooth("norm", "tail_partial_missing", out["norm"], ref["norm"], alt["norm"])
    _report(rep, "voxels %s" % caller)
    problems = _problems(rep, ("tail_partial_missing",))
    assert not problems, "\n".join(problems)


@pytest.mark.parametrize("n,caller,regimes", [(1025, "train", ("value_clip", "norm_clip", "no_clip", "window")),
                                              (263428, "train_wd", ("norm_clip", "value_clip", "at_clip", "zero")),
                                              (262145, "regression", ("no_clip", "value_clip", "zero", "norm_clip"))])
def test_clip_adam_trajectory(n, caller, regimes):
    """Several steps on the kernel's own buffers: each is checked from the state the previous one left."""
    rep = orf.new_report()
    p, _, m, v = _case(n, "zero", caller, 1, 5)
    for step in range(1, 7):
        g = orf.make_grads(n, regimes[step % len(regimes)], 31 * step + n).to(dev())
        out, partial = _launch(p, g, m, v, step, caller, lr=LR * 0.9 ** step)
        _check(rep, "trajectory %s step %d" % (caller, step), p, g, m, v, step, caller, out, partial,
               lr=LR * 0.9 ** step)
        p, m, v = out["p"], out["m"], out["v"]
    _report(rep, "trajectory %s" % caller)
    problems = _problems(rep, ())
    assert not problems, "\n".join(problems)


@pytest.mark.parametrize("n", [1, 1025, 262145])
def test_clip_adam_unbounded_overflowing_norm(n):
    """RegressionEngine's +inf bounds with gradients whose f32 sum of squares overflows: the norm is
    +inf, the coefficient 1, and the step that of unclipped Adam (finite; v ~ 1e37 stays in range)."""
    rep = orf.new_report()
    gen = torch.Generator().manual_seed(n)
    g = (torch.randn(n, generator=gen) * 1e20).float()
    g[0] = 2e20
    p, m, v = orf.make_state(n, 3, n)
    p, g, m, v = (x.to(dev()) for x in (p, g, m, v))
    out, partial = _launch(p, g, m, v, 3, "regression")
    assert float(out["norm"]) == float("inf")
    assert bool(torch.isfinite(out["p"]).all()) and bool(torch.isfinite(out["m"]).all()), \
        "an overflowing norm with max_norm = +inf must leave Adam's step finite"
    _check(rep, "overflow n=%d" % n, p, g, m, v, 3, "regression", out, partial, teeth=False)
    _report(rep, "overflow n=%d" % n)
    problems = _problems(rep, ())
    assert not problems, "\n".join(problems)


def test_clip_adam_two_launches_same_bits():
    p, g, m, v = _case(263428, "norm_clip", "train_wd", 10, 9)
    a, _ = _launch(p, g, m, v, 10, "train_wd")
    b, _ = _launch(p, g, m, v, 10, "train_wd")
    for o in orf.OUTS:
        assert torch.equal(a[o].view(torch.int32), b[o].view(torch.int32)), o


# ----------------------------------------------------------------------------------- the engines
def _snapshot(monkeypatch):
    """Replaces ops.clip_adam with a wrapper that records K7's inputs and then runs it."""
    import fourier_feature_nets_amd as ffn
    real = ffn.ops.clip_adam
    seen = []

    def adam(params, grads, exp_avg, exp_avg_sq, step, lr, **kw):
        seen.append(dict(p=params.clone(), g=grads.clone(), m=exp_avg.clone(), v=exp_avg_sq.clone(), step=step,
                         lr=lr, kw=dict(kw), scratch=kw.get("scratch")))
        real(params, grads, exp_avg, exp_avg_sq, step, lr, **kw)
        seen[-1]["out"] = dict(grads=grads.clone(), m=exp_avg.clone(), v=exp_avg_sq.clone(), p=params.clone(),
                               norm=(kw["norm_out"].clone() if kw.get("norm_out") is not None else None))

    monkeypatch.setattr(ffn.ops, "clip_adam", adam)
    return seen


def _check_engine_step(rep, key, s, a):
    p, g, m, v = s["p"], s["g"], s["m"], s["v"]
    n = p.numel()
    assert s["scratch"] is not None and s["scratch"].numel() >= orf.blocks_of(n)
    out = s["out"]
    want = orf.emulate(p.cpu().numpy(), g.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy(), a)
    if out["norm"] is None:         # (RegressionEngine passes no norm output: nothing to compare there)
        out = dict(out, norm=torch.from_numpy(want["norm"]))
    orf.check_bits(rep, key, out, want)
    orf.check(rep, key, p, g, m, v, a, out, teeth=False)


def test_train_engine_steps_against_the_reference(monkeypatch):
    """Two TrainEngine.train_step calls: K7 gets step counts 1, 2, the caller's lr, wd and 0.1 / 0.1 bounds,
    and the flat buffer / moments it leaves are the reference's."""
    import contextlib
    import io
    import os
    import fourier_feature_nets_amd as ffn
    scene = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scene16.npz")
    torch.manual_seed(7)
    model = ffn.PositionalFourierMLP(3, 4, 5.5, num_channels=64, embedding_size=48).to(dev())
    with contextlib.redirect_stdout(io.StringIO()):
        train = ffn.ImageDataset.load(scene, "train", 16, True, True, device=dev())
    train.sampler.noise_source = "host"
    engine = ffn.TrainEngine(model, weight_decay=1e-3)
    seen = _snapshot(monkeypatch)
    batch = torch.arange(0, len(train), 5, device=dev())
    rep = orf.new_report()
    for it, lr in enumerate((5e-4, 4e-4)):
        engine.train_step(train, batch, it, lr)
        torch.cuda.synchronize()
        s = seen[-1]
        assert s["step"] == it + 1 and s["lr"] == lr
        assert torch.equal(s["out"]["p"], engine.flat)
        a = orf.kernel_args(s["step"], lr, weight_decay=1e-3)
        _check_engine_step(rep, "TrainEngine step %d" % (it + 1), s, a)
        if it:
            assert torch.equal(s["p"], seen[0]["out"]["p"]) and torch.equal(s["m"], seen[0]["out"]["m"])
    _report(rep, "TrainEngine")
    problems = _problems(rep, ())
    assert not problems, "\n".join(problems)


def test_regression_engine_steps_against_the_reference(monkeypatch):
    import fourier_feature_nets_amd as ffn
    torch.manual_seed(4)
    model = ffn.PositionalFourierMLP(2, 3, 6, num_channels=64, embedding_size=64).to(dev())
    gen = torch.Generator().manual_seed(4)
    uv3 = torch.nn.functional.pad(torch.rand((2000, 2), generator=gen) * 2, (0, 1)).to(dev()).contiguous()
    target = torch.rand((2000, 3), generator=gen).to(dev())
    engine = ffn.RegressionEngine(model, weight_decay=1e-3)
    seen = _snapshot(monkeypatch)
    rep = orf.new_report()
    for step in (1, 2, 3):
        lr = 1e-3 * 0.1 ** (step / 2500)
        engine.step(uv3, target, lr)
        torch.cuda.synchronize()
        s = seen[-1]
        assert s["step"] == step and s["lr"] == lr
        assert torch.equal(s["out"]["p"], engine.flat)
        a = orf.kernel_args(step, lr, **orf.CALLERS["regression"])
        _check_engine_step(rep, "RegressionEngine step %d" % step, s, a)
    _report(rep, "RegressionEngine")
    problems = _problems(rep, ())
    assert not problems, "\n".join(problems)
