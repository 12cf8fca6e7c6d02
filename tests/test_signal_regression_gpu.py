"""1-D signal regression on the GPU: K11b (the linear MSE of csrc/regression.hip) against float64
with error budgets and bit for bit against torch.autograd, with its refusals and determinism;
RegressionEngine's coupled weight decay and its freedom from host syncs; 0-d output biases through
forward, backward, the engine and keep_activations; a replay of the reference's own
train_signal_regression runs (tests/golden/signal_regression.npz); the arrays SignalDataset.plot
draws; and scripts/train_signal_regression.py end to end.

Error budgets follow tests/composite_reference.py: an element is held to kappa * 2^-24 * budget,
the budget being a first-order f32 error bound of that element (see each helper).
"""

import argparse
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import fourier_feature_nets_amd as ffn
from fourier_feature_nets_amd import _lib, ops

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
U = 2.0 ** -24
# measured once on an MI355X; the worst ratio over all cases is in brackets
KAPPA_D = 1.0              # d_logits of K11b (three roundings: the bound itself) [0.909, n=63 c=4]
KAPPA_SSE = 1.0            # K11b sums of squares, loss                       [0.153, n=1 c=4]


def dev():
    return torch.device("cuda:0")


def _driver():
    from scripts import train_signal_regression
    return train_signal_regression


# ----------------------------------------------------------------------------------- K11b
def _case(n, c, seed):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn((n, 4), generator=g) * 3
    target = torch.randn((n, c), generator=g) * 2
    k = min(n, 4)
    target[:k, 0] = logits[:k, 0]                # exact zeros of the residual
    return logits.to(dev()), target.to(dev())


def _run_train(logits, target):
    n, c = target.shape
    d_logits = torch.full((n, 4), float("nan"), device=dev())
    partials = torch.full((ops.regression_blocks(n),), float("nan"), device=dev())
    ops.regression_mse_train(logits, target, d_logits, partials)
    loss = torch.full((), float("nan"), device=dev())
    sse = torch.full((), float("nan"), device=dev())
    ops.regression_mse_loss(partials, n * c, sse_out=sse, loss_out=loss)
    return d_logits, partials, float(sse), float(loss)


def _mse_reference(logits, target, scale=1.0):
    """d_logits, per-element budget, sse, sse budget in float64.  d = fl(1/N) (2 fl(z - y)):
    three roundings of |2 r / N| (the residual, 1/N, the product).  Sum of squares: 3 r^2 per
    term (residual and square) plus ceil(log2 n) + 10 levels of summation."""
    n, c = target.shape
    r = logits[:, :c].double() - target.double()
    d = scale * 2 * r / (n * c)
    bud = 3 * 2 * r.abs() / (n * c) + 2.0 ** -149 / U
    sse = float((r * r).sum())
    sse_bud = float(3 * (r * r).sum() + (math.ceil(math.log2(n)) + 10) * (r * r).sum())
    return d, bud, sse, sse_bud


@pytest.mark.parametrize("n", [1, 63, 65, 257, 65541])
@pytest.mark.parametrize("c", [1, 3, 4])
def test_mse_train_against_float64(n, c):
    """d_logits, the partial sums and the loss (sse / count, no 0.5) of K11b within their budgets
    (outputs NaN-filled first: every element is written); columns >= c exactly +0; the evaluation
    pass writes the same partials; two runs give the same bits."""
    logits, target = _case(n, c, 100 * n + c)
    d, partials, sse, loss = _run_train(logits, target)
    ref, bud, sse64, sse_bud = _mse_reference(logits, target)
    ratio = float(((d[:, :c].double() - ref).abs() / (U * bud)).max())
    print("K11b n=%d c=%d d ratio %.3f sse ratio %.3f"
          % (n, c, ratio, abs(sse - sse64) / max(U * sse_bud, 1e-300)))
    assert ratio <= KAPPA_D, (n, c, ratio)
    assert not d[:, c:].any() and not torch.signbit(d[:, c:]).any()
    assert abs(sse - sse64) <= KAPPA_SSE * U * sse_bud, (sse, sse64)
    ref_loss = sse64 / (n * c)
    assert abs(loss - ref_loss) <= KAPPA_SSE * U * (sse_bud / (n * c) + 2 * ref_loss), (loss, ref_loss)
    partials_eval = torch.full_like(partials, float("nan"))
    ops.regression_mse_eval(logits, target, partials_eval)
    assert torch.equal(partials_eval, partials)
    d2, partials2, sse2, loss2 = _run_train(logits, target)
    assert torch.equal(d, d2) and torch.equal(partials, partials2) and sse == sse2 and loss == loss2
    # teeth: K11's 0.5 factor (or a doubled gradient) breaks the bound
    if n > 1:
        for scale in (0.5, 2.0):
            bad, _, _, _ = _mse_reference(logits, target, scale)
            assert float(((d[:, :c].double() - bad).abs() / (U * bud)).max()) > KAPPA_D, scale


@pytest.mark.parametrize("n", [1, 32, 33, 1000, 65541])
@pytest.mark.parametrize("c", [1, 4])
def test_mse_d_logits_are_autograds_bits(n, c):
    """d_logits equal torch.autograd's gradient of (z[:, :c] - y).square().mean() on the same GPU
    tensors bit for bit (columns >= c included).  This test is also where ATen's order for the
    mean backward was worked out: of the two candidates, fl(1/N) * (2 r) and fl((2 r) / N), only
    the first is autograd's -- at counts N that are not powers of two the second differs."""
    logits, target = _case(n, c, 7 * n + c)
    z = logits.clone().requires_grad_()
    (z[:, :c] - target).square().mean().backward()
    d, _, _, _ = _run_train(logits, target)
    assert torch.equal(d, z.grad), (n, c)
    r = logits[:, :c] - target
    count = n * c
    by_reciprocal = torch.tensor(ops.inv_count(count), device=dev()) * (2 * r)
    # (torch's own division by a Python scalar multiplies by the reciprocal on the GPU: the
    # correctly rounded quotient comes from float64)
    by_division = ((2 * r).double() / count).float()
    assert torch.equal(by_reciprocal, z.grad[:, :c])
    if count >= 1000 and count & (count - 1):
        assert not torch.equal(by_division, z.grad[:, :c])


def test_mse_refusals_launch_nothing():
    logits, target = _case(65, 3, 1)
    d = torch.full((65, 4), 5.0, device=dev())
    p = torch.full((ops.regression_blocks(65),), 5.0, device=dev())
    c_i64, c_i, c_f, c_p = _lib.c_i64, _lib.c_i, _lib.c_f, _lib.c_p
    stream = c_p(torch.cuda.current_stream().cuda_stream)
    L, T, D, P = (c_p(t.data_ptr()) for t in (logits, target, d, p))
    bad_train = [(L, T, c_i64(0), c_i(3), D, P), (L, T, c_i64(-4), c_i(3), D, P),
                 (L, T, c_i64(65), c_i(0), D, P), (L, T, c_i64(65), c_i(5), D, P),
                 (L, c_p(0), c_i64(65), c_i(3), D, P), (c_p(0), T, c_i64(65), c_i(3), D, P),
                 (L, T, c_i64(65), c_i(3), c_p(0), P), (L, T, c_i64(65), c_i(3), D, c_p(0))]
    for lg, tg, n, c, dd, pp in bad_train:
        with pytest.raises(_lib.FfnError):
            _lib.call("ffn_regression_mse_train", lg, tg, n, c, c_f(1.0), dd, pp, stream)
    bad_eval = [(L, T, c_i64(0), c_i(3), P), (L, T, c_i64(65), c_i(7), P),
                (c_p(0), T, c_i64(65), c_i(3), P), (L, c_p(0), c_i64(65), c_i(3), P),
                (L, T, c_i64(65), c_i(3), c_p(0))]
    for lg, tg, n, c, pp in bad_eval:
        with pytest.raises(_lib.FfnError):
            _lib.call("ffn_regression_mse_eval", lg, tg, n, c, pp, stream)
    for args in [(P, c_i(0), c_f(1.0), D, D), (c_p(0), c_i(1), c_f(1.0), D, D),
                 (P, c_i(1), c_f(1.0), c_p(0), c_p(0))]:
        with pytest.raises(_lib.FfnError):
            _lib.call("ffn_regression_mse_loss", *args, stream)
    torch.cuda.synchronize()
    assert bool((d == 5).all()) and bool((p == 5).all())


def test_k11_keeps_its_bits_beside_k11b():
    """K11's loss (0.5 * sse / count) is unchanged by the shared final-sum kernel: it equals the
    f32 expression on K11's own sse, and K11b's loss on the same partials is twice it."""
    logits, target = _case(1000, 3, 5)
    partials = torch.empty((ops.regression_blocks(1000),), device=dev())
    ops.regression_train(logits, target, torch.empty((1000, 4), device=dev()), partials)
    sse, half = torch.empty((), device=dev()), torch.empty((), device=dev())
    ops.regression_loss(partials, 3000, sse_out=sse, loss_out=half)
    full = torch.empty((), device=dev())
    ops.regression_mse_loss(partials, 3000, loss_out=full)
    f32 = np.float32
    assert float(half) == float(f32(0.5) * (f32(float(sse)) / f32(3000)))
    assert float(full) == float(f32(float(sse)) / f32(3000)) == 2 * float(half)


# ----------------------------------------------------------------------------------- models, 0-d bias
def _signal_model(fourier, seed=3, channels=64, layers=1, zero_d=True):
    torch.manual_seed(seed)
    ds = ffn.SignalDataset.create(_driver().multifreq, 32, 8)
    args = argparse.Namespace(fourier=fourier, num_samples=32, num_channels=channels,
                              num_layers=layers)
    model = _driver().build_model(args, ds)
    if not zero_d:
        model.layers[-1].bias.data = model.layers[-1].bias.data.reshape(1)
    return model.to(dev()), ds.to(dev())


@pytest.mark.parametrize("fourier", [False, True])
def test_zero_d_bias_equals_a_one_element_bias(fourier):
    """A 0-d output bias (train_signal_regression.py:126) gives the outputs, gradients (0-d for the
    bias), keep_activations slabs and engine updates of the same model with a (1,) bias."""
    m0, ds = _signal_model(fourier, layers=2)
    m1, _ = _signal_model(fourier, layers=2, zero_d=False)
    assert m0.layers[-1].bias.dim() == 0 and tuple(m1.layers[-1].bias.shape) == (1,)
    x = ds.val_x
    with torch.no_grad():
        assert torch.equal(m0(x), m1(x))
    out0, out1 = m0(x), m1(x)
    assert torch.equal(out0, out1)
    g = torch.randn(out0.shape, generator=torch.Generator().manual_seed(2)).to(dev())
    (out0 * g).sum().backward()
    (out1 * g).sum().backward()
    assert m0.layers[-1].bias.grad.shape == () and m1.layers[-1].bias.grad.shape == (1,)
    for a, b in zip(m0.parameters(), m1.parameters()):
        if a.grad is not None:
            assert torch.equal(a.grad.reshape(-1), b.grad.reshape(-1))
    for m in (m0, m1):
        m.keep_activations = True
        with torch.no_grad():
            m(x)
        m.keep_activations = False
    assert np.array_equal(m0.activations[-1], m1.activations[-1])
    e0 = ffn.RegressionEngine(m0, weight_decay=1e-3, loss="linear")
    e1 = ffn.RegressionEngine(m1, weight_decay=1e-3, loss="linear")
    for _ in range(3):
        l0 = e0.step(ds.train_x3, ds.train_y, 5e-4)
        l1 = e1.step(ds.train_x3, ds.train_y, 5e-4)
        assert torch.equal(l0, l1)
    assert torch.equal(e0.flat, e1.flat)
    assert m0.layers[-1].bias.dim() == 0 and m0.layers[-1].bias.data_ptr() != 0
    assert torch.equal(e0.validation_loss(ds.val_x3, ds.val_y), e1.validation_loss(ds.val_x3, ds.val_y))


def test_wrong_device_or_size_bias_is_refused_before_any_launch():
    """A host tensor assigned to a GPU model's bias (the reference's assignment done after .to())
    and a bias of the wrong size raise before the pack table copies from its pointer."""
    model, ds = _signal_model(False)
    orig = model.layers[-1].bias.data
    with torch.no_grad():
        before = model(ds.val_x).clone()
    model.layers[-1].bias.data = torch.tensor(1.5)                  # on the host
    with pytest.raises(RuntimeError, match="lives on cpu"):
        model(ds.val_x)
    with pytest.raises(RuntimeError, match="lives on cpu"):
        ffn.RegressionEngine(model, loss="linear")
    model.layers[-1].bias.data = torch.zeros(3, device=dev())
    with pytest.raises(ValueError, match="bias of shape"):
        model(ds.val_x)
    # once the bias is back on the model's device, the model computes again
    model.layers[-1].bias.data = orig
    with torch.no_grad():
        assert torch.equal(model(ds.val_x), before)


# ----------------------------------------------------------------------------------- RegressionEngine
def test_engine_weight_decay_is_k7s_formula_bit_for_bit():
    """With weight_decay the update is K7's formula including + wd * p, op by op in f32, bit for
    bit, over three steps; the gradient buffer keeps the raw gradient; the loss equals
    mean((z - y)^2) of the pre-update weights (float64, 1e-5 relative)."""
    model, ds = _signal_model(True)
    wd = 1e-3
    engine = ffn.RegressionEngine(model, weight_decay=wd, loss="linear")
    f32 = lambda v: torch.tensor(v, dtype=torch.float32, device=dev())   # noqa: E731
    b1, b2, eps, wdt = f32(0.9), f32(0.999), f32(1e-8), f32(wd)
    lr = 5e-4
    for step in range(1, 4):
        p0, m0, v0 = engine.flat.clone(), engine.exp_avg.clone(), engine.exp_avg_sq.clone()
        with torch.no_grad():
            out = model(ds.train_x)
        loss = engine.step(ds.train_x3, ds.train_y, lr)
        g = engine.grads + wdt * p0
        m = m0 + (g - m0) * (f32(1.0) - b1)
        v = v0 * b2 + ((f32(1.0) - b2) * g) * g
        step_size = f32(lr / (1.0 - 0.9 ** step))
        inv_sqrt_bc2 = f32(1.0 / math.sqrt(1.0 - 0.999 ** step))
        p = p0 - step_size * (m / (torch.sqrt(v) * inv_sqrt_bc2 + eps))
        assert torch.equal(engine.exp_avg, m) and torch.equal(engine.exp_avg_sq, v), step
        assert torch.equal(engine.flat, p), step
        # teeth: the same formula without the decay term is a different update
        m_plain = m0 + (engine.grads - m0) * (f32(1.0) - b1)
        assert not torch.equal(m_plain, m)
        ref = float(((out.double() - ds.train_y.double()) ** 2).mean())
        assert abs(float(loss) - ref) <= 1e-5 * ref


def test_engine_linear_step_issues_no_host_sync():
    model, ds = _signal_model(True)
    engine = ffn.RegressionEngine(model, weight_decay=1e-3, loss="linear")
    engine.step(ds.train_x3, ds.train_y, 5e-4)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        losses = [engine.step(ds.train_x3, ds.train_y, 5e-4) for _ in range(5)]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    vals = [float(x) for x in losses]
    assert all(math.isfinite(v) for v in vals) and vals[-1] < vals[0]
    with pytest.raises(ValueError):
        ffn.RegressionEngine(model, loss="l1")


# ----------------------------------------------------------------------------------- reference replay
RUNS = ["multifreq", "multifreq_fourier", "sawtooth_fourier", "triangle"]
# per run: (every step's training loss, relative; the reports' validation losses, relative; the
# weights after the last update, absolute) -- about twice the worst deviation measured once on an
# MI355X, see test_replays_the_reference_signal_regression
TOLERANCES = {"multifreq": (2e-3, 3e-3, 2e-2),
              "multifreq_fourier": (0.5, 0.3, 2e-2),
              "sawtooth_fourier": (7e-2, 5e-3, 5e-2),
              "triangle": (1e-2, 1e-2, 3e-3)}
TOL_FIRST_1000 = 1e-2      # every run's training loss over steps 0..1000, relative


def _replay(g, run, num_steps):
    argv = json_list(g[run + "/args"])
    args = argparse.Namespace(fourier="--fourier" in argv, num_samples=32, num_channels=64,
                              num_layers=1)
    ds = ffn.SignalDataset.create(_driver().SIGNALS[argv[0]], 32, 8)
    model = _driver().build_model(args, ds)
    model.load_state_dict({k[len(run) + 6:]: torch.from_numpy(g[k]) for k in g.files
                           if k.startswith(run + "/init/")})
    model = model.to(dev())
    engine = ffn.RegressionEngine(model, weight_decay=1e-3, loss="linear")
    losses = []
    log = _driver().train_loop(engine, ds.to(dev()), num_steps, losses=losses)
    state = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    return np.array([float(x) for x in torch.stack(losses).cpu()]), log, state


def json_list(a):
    import json
    return json.loads(str(a))


@pytest.mark.parametrize("run", RUNS)
def test_replays_the_reference_signal_regression(run):
    """The reference's own train_signal_regression runs (CPU, seeded, --no-plot, the default 10 000
    steps; tests/golden/signal_regression.npz) replayed from their initial state through the
    driver's loop.  The reference computes on the CPU, so every step differs in the last bits and
    Adam carries the differences along.  Checked: every step's training loss, the report lines'
    steps and format, their training and validation losses, and the weights after the last update.

    The full 10 000-step default holds, with tolerances that follow how far last-bit differences
    carry.  Worst deviations measured once on an MI355X, in brackets:
    - training loss over steps 0..1000, relative: 1e-2 [5.0e-3, sawtooth_fourier];
    - training loss over all steps, relative: multifreq 2e-3 [8.0e-4], multifreq_fourier 0.5
      [0.22], sawtooth_fourier 7e-2 [3.3e-2], triangle 1e-2 [4.0e-3].  multifreq_fourier fits
      the signal down to a loss of ~3e-6, where Adam's steps of ~lr on weights whose gradients
      are near zero move the loss by tens of percent whatever their last bits are;
    - validation losses at the reports, relative: 3e-3 [1.1e-3], 0.3 [0.15], 5e-3 [2.3e-3],
      1e-2 [5.5e-3]; the final ones agree to 4 % or better [3.3e-6 vs 3.5e-6, multifreq_fourier];
    - final weights, absolute: 2e-2 [8.1e-3], 2e-2 [7.3e-3], 5e-2 [2.4e-2], 3e-3 [1.2e-3]."""
    g = np.load(os.path.join(GOLDEN, "signal_regression.npz"))
    num_steps = int(g["num_steps"])
    losses, log, state = _replay(g, run, num_steps)
    ref_loss = g[run + "/loss"].astype(np.float64)
    assert len(losses) == len(ref_loss) == num_steps + 1
    rel = np.abs(losses / ref_loss - 1)
    ref_val = g[run + "/report_val"]
    val_rel = np.abs(np.array([e[2] for e in log]) / ref_val - 1)
    final = "%s/state%d/" % (run, num_steps)
    dstate = max(float(np.max(np.abs(state[k[len(final):]] - g[k]))) for k in g.files
                 if k.startswith(final))
    worst = {"loss_rel": float(rel.max()), "loss_rel_first_1000": float(rel[:1001].max()),
             "val_rel": float(val_rel.max()), "state_abs": dstate,
             "final_val": (log[-1][2], float(ref_val[-1]))}
    print("signal regression replay %s worst deviations %s" % (run, worst))
    assert [e[0] for e in log] == g[run + "/report_step"].tolist()
    lines = [" ".join(str(v) for v in (e[0], "train:", e[1], "val:", e[2])) for e in log]
    for mine, ref in zip(lines, g[run + "/report_lines"]):
        assert [t for t in mine.split() if not t[0].isdigit()] == \
               [t for t in str(ref).split() if not t[0].isdigit()]
        assert re.fullmatch(r"\d+ train: \S+ val: \S+", mine), mine
    assert np.array_equal(np.array([e[1] for e in log], np.float32),
                          losses[g[run + "/report_step"]].astype(np.float32))
    tol_loss, tol_val, tol_state = TOLERANCES[run]
    assert rel[:1001].max() <= TOL_FIRST_1000, worst
    assert rel.max() <= tol_loss, worst
    assert val_rel.max() <= tol_val, worst
    assert dstate <= tol_state, worst


# ----------------------------------------------------------------------------------- plot
PLOT_BUDGET = 1e-4         # absolute, on values of order 1


def _plot_model(g):
    run, n = "multifreq_fourier", int(g["num_steps"])
    args = argparse.Namespace(fourier=True, num_samples=32, num_channels=64, num_layers=1)
    ds = ffn.SignalDataset.create(_driver().multifreq, 32, 8)
    model = _driver().build_model(args, ds)
    pre = "%s/state%d/" % (run, n)
    model.load_state_dict({k[len(pre):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(pre)})
    return ds, model.to(dev())


def test_plot_arrays_match_what_the_reference_draws():
    """SignalDataset._plot_arrays on the reference run's final weights against the arrays the
    reference's plot drew (tests/golden/make_signal_regression.py): x exactly, predictions and the
    drawn units' lines within PLOT_BUDGET, the drawn units in the reference's order wherever
    neighbouring ranges differ by more than the budget, the on-masks away from ties; and, with
    matplotlib, the axes plot() fills carry these arrays."""
    g = np.load(os.path.join(GOLDEN, "signal_regression.npz"))
    ds, model = _plot_model(g)
    arr = ds._plot_arrays(model, 48, 10)
    pred = g["plot/pred"]
    assert np.array_equal(arr["x_vals"].astype(np.float64), pred[:, 0])
    assert np.max(np.abs(arr["y_vals"] - pred[:, 1])) <= PLOT_BUDGET
    labels = [str(s) for s in g["plot/labels"]]
    ref_index = [int(s[1:]) for s in labels]
    ranges = arr["activation_range"]
    mine = list(arr["index"])
    assert len(mine) == len(ref_index) == 10
    sorted_ranges = np.sort(ranges)[::-1]
    for k in range(10):
        separated = (k == 0 or sorted_ranges[k - 1] - sorted_ranges[k] > PLOT_BUDGET) and \
                    (sorted_ranges[k] - sorted_ranges[k + 1] > PLOT_BUDGET)
        if separated:
            assert mine[k] == ref_index[k], (k, mine, ref_index)
    for k, i in enumerate(ref_index):
        line = g["plot/hidden_line%d" % k]
        assert np.array_equal(line[:, 0], pred[:, 0])
        assert np.max(np.abs(arr["activation_values"][:, i] - line[:, 1])) <= PLOT_BUDGET
        on_ref = np.isin(pred[:, 0], g["plot/hidden_scatter%d" % k][:, 0])
        on = arr["activation"][:, i] > 0
        clear = np.abs(arr["activation"][:, i]) > PLOT_BUDGET
        assert np.array_equal(on[clear], on_ref[clear]), k
    assert np.allclose(arr["hidden_ylim"], g["plot/hidden_ylim"], rtol=0, atol=2 * PLOT_BUDGET)
    pytest.importorskip("matplotlib")
    from matplotlib.figure import Figure
    fig = Figure(figsize=(12.8, 7.2), dpi=100)
    hidden_ax, space_ax = fig.add_subplot(121), fig.add_subplot(122)
    ds.plot(space_ax, hidden_ax, model, 48, g["plot/colors"], 10)
    assert [ln.get_label() for ln in hidden_ax.lines] == ["h{:02d}".format(i) for i in mine]
    for k, i in enumerate(mine):
        assert np.array_equal(hidden_ax.lines[k].get_xydata()[:, 1],
                              arr["activation_values"][:, i].astype(np.float64))
        assert len(hidden_ax.collections[k].get_offsets()) == int(arr["on"][k].sum())
    assert np.array_equal(space_ax.lines[0].get_xydata(), g["plot/val_line"])
    assert np.array_equal(space_ax.lines[1].get_xydata(), g["plot/train_line"])
    assert np.max(np.abs(space_ax.collections[0].get_offsets() - pred)) <= PLOT_BUDGET
    assert np.allclose(space_ax.get_xlim(), g["plot/space_xlim"], rtol=0, atol=0)
    assert np.allclose(space_ax.get_ylim(), g["plot/space_ylim"], rtol=0, atol=0)
    assert np.allclose(hidden_ax.get_ylim(), g["plot/hidden_ylim"], rtol=0, atol=2 * PLOT_BUDGET)


# ----------------------------------------------------------------------------------- driver script
def _run_driver(out, *extra):
    return subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train_signal_regression.py"),
                           "multifreq", out, "--num-steps", "60", "--num_plot", "16",
                           "--resolution", "320x240"] + list(extra),
                          capture_output=True, text=True, cwd=ROOT, timeout=300)


def test_train_signal_regression_script(tmp_path):
    """scripts/train_signal_regression.py: report lines in the reference's format at steps 0, 50
    and 60, log.txt with the reference's header and the same numbers, PNG frames per report unless
    --no-plot, and --make-video warns on stderr and writes the frames."""
    from PIL import Image
    plain = str(tmp_path / "plain")
    res = _run_driver(plain, "--no-plot", "--fourier")
    assert res.returncode == 0, res.stderr[-2000:]
    lines = res.stdout.strip().splitlines()
    assert [int(ln.split()[0]) for ln in lines] == [0, 50, 60]
    for ln in lines:
        assert re.fullmatch(r"\d+ train: \d\.\d+(e-\d+)? val: \d\.\d+(e-\d+)?", ln), ln
    with open(os.path.join(plain, "log.txt")) as f:
        log = f.read().splitlines()
    assert log[0] == "step\ttrain_loss\tval_loss"
    assert log[1:] == ["\t".join(ln.split()[i] for i in (0, 2, 4)) for ln in lines]
    assert not [f for f in os.listdir(plain) if f.endswith(".png")]
    assert "make-video" not in res.stderr
    video = str(tmp_path / "video")
    res = _run_driver(video, "--no-plot", "--make-video")
    assert res.returncode == 0, res.stderr[-2000:]
    assert "warning: --make-video" in res.stderr
    frames = sorted(f for f in os.listdir(video) if f.endswith(".png"))
    assert frames == ["frame_00000.png", "frame_00001.png", "frame_00002.png"]
    img = np.asarray(Image.open(os.path.join(video, frames[-1])))
    assert img.shape == (240, 320, 3) and img.std() > 0
