"""2-D image regression on the GPU: 1- and 2-input FourierFeatureMLP chains (all four families)
against float64 and against the equivalent 3-input chain; K11 (csrc/regression.hip) against
float64 with error budgets, with its refusals and determinism; RegressionEngine's Adam step and its
freedom from host syncs; a replay of the reference's own train_image_regression run
(tests/golden/image_regression.npz); and scripts/train_image_regression.py end to end.

Error budgets follow tests/composite_reference.py: an element is held to kappa * 2^-24 * budget,
the budget being a first-order f32 error bound of that element (see each helper).
"""

import contextlib
import io
import json
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
# measured once on an MI355X; the worst ratio over all cases is in brackets.  The forward budget
# sums every product's worst case through the layers, so real errors sit far below it.
KAPPA_FORWARD = 0.05       # model outputs, D in {1, 2}   [0.017, mlp D=1]
KAPPA_SIGMOID = 4.0        # d_logits of K11              [1.90, n=65541 c=3]
KAPPA_SSE = 1.0            # K11 sums of squares, loss    [0.037, n=63 c=4]


def dev():
    return torch.device("cuda:0")


# ----------------------------------------------------------------------------------- models, D < 3
FAMILIES = {
    "mlp": lambda d: ffn.MLP(d, 3, num_channels=64),
    "basic": lambda d: ffn.BasicFourierMLP(d, 3, num_channels=96),
    "positional": lambda d: ffn.PositionalFourierMLP(d, 3, 6, num_channels=256, embedding_size=256),
    "gaussian": lambda d: ffn.GaussianFourierMLP(d, 4, 10.0, num_channels=128, embedding_size=96),
}


def _forward64(model, x):
    """fourier_feature_models.py:57-78 in float64, with a first-order f32 error budget per
    output: features |a| (sum_d |pi x_d b_dk| + 1) (angle rounding, sin/cos), raw inputs |x|;
    each layer |W| budget_in + |W| |h_in| + |b| (products and sums; ReLU passes errors through)."""
    x = x.double()
    if model.b_values is None:
        h, bud = x, x.abs()
    else:
        b = model.b_values.data.double()
        a = model.a_values.data.double()
        ang = (math.pi * x) @ b
        h = torch.cat([a * ang.cos(), a * ang.sin()], -1)
        mag = (math.pi * x).abs() @ b.abs() + 1
        bud = torch.cat([a.abs() * mag, a.abs() * mag], -1)
    for i, layer in enumerate(model.layers):
        w, bias = layer.weight.data.double(), layer.bias.data.double()
        z = h @ w.T + bias
        bud = bud @ w.abs().T + h.abs() @ w.abs().T + bias.abs()
        h = torch.relu(z) if i < len(model.layers) - 1 else z
    return h, bud


def _inputs(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((n, d), generator=g) * 2).to(dev())


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("d", [1, 2])
def test_low_dimensional_forward_against_float64(family, d):
    """Outputs within kappa * 2^-24 * budget of float64, for ragged batch sizes; the reference
    at inputs scaled by 1 + 1e-3 must break the bound.  Fails on the parent commit with
    NotImplementedError (the chain covered 3 inputs only)."""
    torch.manual_seed(11 + d)
    model = FAMILIES[family](d).to(dev())
    worst = 0.0
    for n in (1, 33, 1000, 4133):
        x = _inputs(n, d, n)
        with torch.no_grad():
            got = model(x).double()
            ref, bud = _forward64(model, x)
        assert got.shape == (n, model.num_outputs)
        ratio = float(((got - ref).abs() / (U * bud)).max())
        worst = max(worst, ratio)
        assert ratio <= KAPPA_FORWARD, (family, d, n, ratio)
    # teeth: a reference evaluated at inputs off by 1e-3 relative (a mis-scaled or mis-mapped
    # input column of the lift) fails the bound
    x = _inputs(1000, d, 5)
    with torch.no_grad():
        got = model(x).double()
        ref, bud = _forward64(model, x * (1 + 1e-3))
    assert float(((got - ref).abs() / (U * bud)).max()) > KAPPA_FORWARD
    print("forward %s D=%d worst ratio %.3f" % (family, d, worst))


def _lifted_copy(model):
    """The same network as a 3-input model: B with zero rows, the plain MLP's first layer with
    zero weight columns for the missing inputs."""
    d = model.num_inputs
    a = None if model.a_values is None else model.a_values.data.cpu()
    b = None if model.b_values is None else torch.cat(
        [model.b_values.data.cpu(), torch.zeros(3 - d, model.b_values.shape[1])])
    channels = [layer.out_features for layer in model.layers[:-1]]
    big = ffn.FourierFeatureMLP(3, model.num_outputs, a, b, channels)
    state = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    if model.b_values is None:
        w = state["layers.0.weight"]
        state["layers.0.weight"] = torch.cat([w, torch.zeros(w.shape[0], 3 - d)], 1)
    else:
        state["a_values"], state["b_values"] = big.a_values.data, big.b_values.data
    big.load_state_dict(state)
    return big.to(dev())


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("d", [1, 2])
def test_low_dimensional_chain_is_the_three_input_chain(family, d):
    """Forward outputs and weight gradients of a D-input model are bit-identical to the 3-input
    model with zero rows of B / zero raw-input columns on zero-padded inputs (the lift of
    EncodingSpec): the kernels see the same chain.  Weight gradients also agree with float64
    autograd (max error <= 1e-4 of the layer's largest gradient) on the samples whose ReLU
    decisions are not within 1e-4 of a tie."""
    torch.manual_seed(3 + d)
    model = FAMILIES[family](d).to(dev())
    big = _lifted_copy(model)
    n = 2085
    x = _inputs(n, d, 9)
    x3 = torch.nn.functional.pad(x, (0, 3 - d))
    g = torch.randn((n, model.num_outputs), generator=torch.Generator().manual_seed(1)).to(dev())
    out = model(x)
    (out * g).sum().backward()
    out3 = big(x3)
    (out3 * g).sum().backward()
    assert torch.equal(out, out3)
    for i, (la, lb) in enumerate(zip(model.layers, big.layers)):
        gw = lb.weight.grad[:, :la.in_features] if (i == 0 and model.b_values is None) else lb.weight.grad
        assert torch.equal(la.weight.grad, gw), (family, d, i)
        assert torch.equal(la.bias.grad, lb.bias.grad), (family, d, i)
    # float64 autograd of the reference formula, on the samples whose hidden pre-activations are
    # all at least 1e-4 away from 0 (elsewhere an f32 ReLU decision may legitimately differ)
    params = [p.detach().double().requires_grad_() for layer in model.layers for p in (layer.weight, layer.bias)]

    def reference(inputs):
        h = inputs.double()
        if model.b_values is not None:
            ang = (math.pi * h) @ model.b_values.data.double()
            a = model.a_values.data.double()
            h = torch.cat([a * ang.cos(), a * ang.sin()], -1)
        margin = torch.full((inputs.shape[0],), float("inf"), dtype=torch.float64, device=dev())
        for i in range(len(model.layers)):
            h = h @ params[2 * i].T + params[2 * i + 1]
            if i < len(model.layers) - 1:
                margin = torch.minimum(margin, h.detach().abs().min(1).values)
                h = torch.relu(h)
        return h, margin

    _, margin = reference(x)
    safe = margin > 1e-4
    assert int(safe.sum()) > n // 2
    xs, gs = x[safe], g[safe]
    model.zero_grad()
    (model(xs) * gs).sum().backward()
    h, _ = reference(xs)
    (h * gs.double()).sum().backward()
    for i, layer in enumerate(model.layers):
        for mine, ref in ((layer.weight.grad, params[2 * i].grad), (layer.bias.grad, params[2 * i + 1].grad)):
            err = float((mine.double() - ref).abs().max())
            assert err <= 1e-4 * float(ref.abs().max()) + 1e-9, (family, d, i, err)


def test_grid_inputs_keep_their_leading_shape():
    """(H, W, 2) uv grids give (H, W, C) outputs equal to the flattened call, and
    keep_activations leaves activations[-1] of shape (H, W, channels) (as the reference's numpy
    copy of a grid-shaped forward has)."""
    torch.manual_seed(0)
    model = ffn.PositionalFourierMLP(2, 3, 6, num_channels=64, embedding_size=64).to(dev())
    uv = ffn.PixelDataset.generate_uvs(24, dev())
    with torch.no_grad():
        grid = model(uv)
        flat = model(uv.reshape(-1, 2))
        model.keep_activations = True
        grid2 = model(uv)
        acts_grid = model.activations[-1]
        model(uv.reshape(-1, 2))
        acts_flat = model.activations[-1]
        model.keep_activations = False
    assert grid.shape == (24, 24, 3) and torch.equal(grid.reshape(-1, 3), flat)
    assert torch.equal(grid2, grid)
    assert acts_grid.shape == (24, 24, 64) and acts_flat.shape == (24 * 24, 64)
    assert np.array_equal(acts_grid.reshape(-1, 64), acts_flat) and acts_flat.any()
    with pytest.raises(ValueError):
        model(torch.zeros((5, 3), device=dev()))


def test_bf16x6_covers_the_lifted_chain():
    """The opt-in f32-accurate bf16x6 mode runs a 2-input chain unchanged (it sees an ordinary
    3-input chain): outputs within the exact-f32 budget of float64."""
    torch.manual_seed(5)
    model = ffn.PositionalFourierMLP(2, 3, 6, num_channels=256, embedding_size=256).to(dev())
    model.precision = "bf16x6"
    assert model.program().covers("bf16x6")
    x = _inputs(3000, 2, 8)
    with torch.no_grad():
        got = model(x).double()
        ref, bud = _forward64(model, x)
    assert float(((got - ref).abs() / (U * bud)).max()) <= KAPPA_FORWARD


def test_load_model_round_trips_a_two_input_checkpoint(tmp_path):
    torch.manual_seed(2)
    model = ffn.GaussianFourierMLP(2, 3, 10.0, num_channels=32, embedding_size=32)
    path = str(tmp_path / "m.pt")
    model.save(path)
    back = ffn.load_model(path)
    assert isinstance(back, ffn.FourierFeatureMLP) and back.num_inputs == 2
    model, back = model.to(dev()), back.to(dev())
    x = _inputs(500, 2, 1)
    with torch.no_grad():
        assert torch.equal(model(x), back(x))


# ----------------------------------------------------------------------------------- K11
def _sigmoid_terms64(logits, target):
    c = target.shape[1]
    z = logits[:, :c].double()
    s = torch.sigmoid(z)
    r = s - target.double()
    return s, r


def _train_reference(logits, target, drop_half=False, drop_sigmoid=False):
    """d_logits, per-element budget, sse, sse budget in float64.
    Budget of d = ((s - y) inv) (1 - s) s with s within 3u s of sigmoid:
      inv ((|r| + s)(1 - s) s + |r| s s + 4 |r| (1 - s) s)   (r, 1 - s, their rounding, 3 products).
    Budget of the sum of squares: sum 2 |r| (|r| + s) + ceil(log2 n + 2) r^2."""
    n, c = target.shape
    inv = 1.0 / (n * c)
    s, r = _sigmoid_terms64(logits, target)
    d = (r * (inv * (2 if drop_half else 1))) * ((1 - s) * s if not drop_sigmoid else 1)
    bud = inv * ((r.abs() + s) * (1 - s) * s + r.abs() * s * s + 4 * r.abs() * (1 - s) * s)
    # sigmoids below the smallest normal f32 (z < -87) flush towards 0: an absolute floor
    bud = bud + inv * (r.abs() + 1) * (2.0 ** -126 / U)
    sse = float((r * r).sum())
    sse_bud = float((2 * r.abs() * (r.abs() + s)).sum() + (math.ceil(math.log2(n)) + 10) * (r * r).sum())
    return d, bud, sse, sse_bud


def _case(n, c, seed):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn((n, 4), generator=g) * 3
    # extremes: saturated sigmoids both ways and exact zeros
    k = min(n, 8)
    logits[:k, 0] = torch.tensor([30.0, -30.0, 100.0, -100.0, 0.0, 17.0, -17.0, 1e-3])[:k]
    target = torch.rand((n, c), generator=g)
    target[:k // 2] = torch.randint(0, 2, (k // 2, c), generator=g).float()
    return logits.to(dev()), target.to(dev())


def _run_train(logits, target):
    n, c = target.shape
    d_logits = torch.full((n, 4), float("nan"), device=dev())
    partials = torch.full((ops.regression_blocks(n),), float("nan"), device=dev())
    ops.regression_train(logits, target, d_logits, partials)
    loss = torch.full((), float("nan"), device=dev())
    sse = torch.full((), float("nan"), device=dev())
    ops.regression_loss(partials, n * c, sse_out=sse, loss_out=loss)
    return d_logits, partials, float(sse), float(loss)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 65541])
@pytest.mark.parametrize("c", [1, 3, 4])
def test_regression_train_against_float64(n, c):
    """d_logits, the partial sums and the loss of K11 within their budgets (outputs NaN-filled
    first: every element is written); columns >= c exactly 0; two runs give the same bits."""
    logits, target = _case(n, c, 100 * n + c)
    d, partials, sse, loss = _run_train(logits, target)
    ref, bud, sse64, sse_bud = _train_reference(logits, target)
    ratio = float(((d[:, :c].double() - ref).abs() / (U * bud + 1e-300)).max())
    assert ratio <= KAPPA_SIGMOID, (n, c, ratio)
    assert not d[:, c:].any() and not torch.signbit(d[:, c:]).any()     # exactly +0
    assert torch.isfinite(partials).all()
    print("K11 n=%d c=%d d_logits ratio %.3f sse ratio %.3f" % (n, c, ratio, abs(sse - sse64) / (U * sse_bud)))
    assert abs(sse - sse64) <= KAPPA_SSE * U * sse_bud, (sse, sse64)
    ref_loss = 0.5 * sse64 / (n * c)
    assert abs(loss - ref_loss) <= KAPPA_SSE * U * (0.5 * sse_bud / (n * c) + 2 * ref_loss), (loss, ref_loss)
    d2, partials2, sse2, loss2 = _run_train(logits, target)
    assert torch.equal(d, d2) and torch.equal(partials, partials2) and sse == sse2 and loss == loss2
    # teeth: the 0.5 factor dropped, or sigmoid's derivative missing, breaks the bound (n = 1 is
    # a single saturated sigmoid: nothing to tell apart)
    for alt in (dict(drop_half=True), dict(drop_sigmoid=True)) if n > 8 else ():
        bad, _, _, _ = _train_reference(logits, target, **alt)
        assert float(((d[:, :c].double() - bad).abs() / (U * bud + 1e-300)).max()) > KAPPA_SIGMOID, alt


@pytest.mark.parametrize("n", [1, 65, 257, 65541])
@pytest.mark.parametrize("c", [1, 3, 4])
def test_regression_eval_against_float64(n, c):
    """Evaluation sums equal the training kernel's bit for bit; the u8 pixels are
    trunc(sigmoid * 255) -- exactly, wherever float64's value is not within 1e-4 of an integer."""
    logits, target = _case(n, c, 7 * n + c)
    _, partials_train, _, _ = _run_train(logits, target)
    partials = torch.full_like(partials_train, float("nan"))
    image = torch.full((n, c), 77, dtype=torch.uint8, device=dev())
    ops.regression_eval(logits, target, c, partials, image)
    assert torch.equal(partials, partials_train)
    s64 = torch.sigmoid(logits[:, :c].double()) * 255
    ref = torch.floor(s64)
    near = (s64 - torch.round(s64)).abs() < 1e-4
    diff = (image.double() - ref).abs()
    assert float(diff[~near].max() if (~near).any() else 0) == 0
    assert float(diff.max()) <= 1
    # image only (no target): same pixels; partials only: same sums
    image2 = torch.zeros_like(image)
    ops.regression_eval(logits, None, c, None, image2)
    assert torch.equal(image, image2)
    partials3 = torch.full_like(partials, float("nan"))
    ops.regression_eval(logits, target, c, partials3, None)
    assert torch.equal(partials3, partials_train)


def test_regression_refusals_launch_nothing():
    logits, target = _case(65, 3, 1)
    d = torch.full((65, 4), 5.0, device=dev())
    p = torch.full((ops.regression_blocks(65),), 5.0, device=dev())
    lib = _lib.load()
    c_i64, c_i, c_f, c_p = _lib.c_i64, _lib.c_i, _lib.c_f, _lib.c_p
    stream = c_p(torch.cuda.current_stream().cuda_stream)
    L, T, D, P = (c_p(t.data_ptr()) for t in (logits, target, d, p))
    bad_train = [(L, T, c_i64(0), c_i(3)), (L, T, c_i64(-4), c_i(3)), (L, T, c_i64(65), c_i(0)),
                 (L, T, c_i64(65), c_i(5)), (L, c_p(0), c_i64(65), c_i(3))]
    for lg, tg, n, c in bad_train:
        with pytest.raises(_lib.FfnError):
            _lib.call("ffn_regression_train", lg, tg, n, c, c_f(1.0), D, P, stream)
    bad_eval = [(T, c_i64(0), c_i(3), P, None), (T, c_i64(65), c_i(7), P, None),
                (c_p(0), c_i64(65), c_i(3), P, None), (T, c_i64(65), c_i(3), c_p(0), c_p(0))]
    for tg, n, c, pp, img in bad_eval:
        with pytest.raises(_lib.FfnError):
            _lib.call("ffn_regression_eval", L, tg, n, c, pp, img if img is not None else c_p(0), stream)
    with pytest.raises(_lib.FfnError):
        _lib.call("ffn_regression_loss", P, c_i(0), c_f(1.0), D, D, stream)
    torch.cuda.synchronize()
    assert bool((d == 5).all()) and bool((p == 5).all())


# ----------------------------------------------------------------------------------- RegressionEngine
def _small_setup(seed=4, n=2000):
    torch.manual_seed(seed)
    model = ffn.PositionalFourierMLP(2, 3, 6, num_channels=64, embedding_size=64).to(dev())
    g = torch.Generator().manual_seed(seed)
    uv3 = torch.nn.functional.pad(torch.rand((n, 2), generator=g) * 2, (0, 1)).to(dev()).contiguous()
    target = torch.rand((n, 3), generator=g).to(dev())
    return model, uv3, target


def test_engine_step_is_unclipped_adam_bit_for_bit():
    """K7 with clip_value = max_norm = +inf is the identity on the gradients: the update equals
    Adam's formula (as K7 writes it, in f32 op by op) on the raw gradients, bit for bit, for
    three steps; the loss equals 0.5 * mean((sigmoid - y)^2) of the pre-update weights."""
    model, uv3, target = _small_setup()
    engine = ffn.RegressionEngine(model)
    f32 = lambda v: torch.tensor(v, dtype=torch.float32, device=dev())   # noqa: E731
    b1, b2, eps = f32(0.9), f32(0.999), f32(1e-8)
    for step in range(1, 4):
        p0, m0, v0 = engine.flat.clone(), engine.exp_avg.clone(), engine.exp_avg_sq.clone()
        with torch.no_grad():
            out = torch.sigmoid(model(uv3[:, :2]))
        lr = 1e-3 * 0.1 ** (step / 2500)
        loss = engine.step(uv3, target, lr)
        g = engine.grads
        m = m0 + (g - m0) * (f32(1.0) - b1)
        v = v0 * b2 + ((f32(1.0) - b2) * g) * g
        step_size = f32(lr / (1.0 - 0.9 ** step))
        inv_sqrt_bc2 = f32(1.0 / math.sqrt(1.0 - 0.999 ** step))
        p = p0 - step_size * (m / (torch.sqrt(v) * inv_sqrt_bc2 + eps))
        assert torch.equal(engine.exp_avg, m) and torch.equal(engine.exp_avg_sq, v), step
        assert torch.equal(engine.flat, p), step
        ref = 0.5 * float(((out.double() - target.double()) ** 2).mean())
        assert abs(float(loss) - ref) <= 1e-5 * ref
    # the weights the model computes with are the engine's buffer
    assert model.layers[0].weight.data_ptr() == engine.flat.data_ptr()


def test_engine_step_issues_no_host_sync():
    model, uv3, target = _small_setup(n=4096)
    engine = ffn.RegressionEngine(model)
    engine.step(uv3, target, 1e-3)               # plans and buffers for this size
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        losses = [engine.step(uv3, target, 1e-3 * 0.1 ** (s / 2500)) for s in range(1, 4)]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    vals = [float(x) for x in losses]
    assert all(math.isfinite(v) for v in vals) and vals[-1] < vals[0]


# ----------------------------------------------------------------------------------- reference replay
def _replay(g, name):
    params = json.loads(str(g[name + "/params"]))
    for key in ("a_values", "b_values"):
        if params[key] is not None:
            params[key] = torch.FloatTensor(params[key])
    model = ffn.FourierFeatureMLP(**params)
    model.load_state_dict({k[len(name) + 6:]: torch.from_numpy(g[k]) for k in g.files
                           if k.startswith(name + "/init/")})
    model = model.to(dev())
    size = int(g["size"])
    dataset = ffn.PixelDataset.from_array(g["image"], "RGB", size).to(dev())
    engine = ffn.RegressionEngine(model)
    steps, report = int(g["num_steps"]), int(g["report_interval"])
    losses, reports = [], []
    lr = 1e-3
    for step in range(steps + 1):
        if step % report == 0 or step == steps:
            sse, _ = engine.evaluate(dataset.val_uv3, dataset.val_color_flat)
            reports.append((step, ffn.PixelDataset.psnr_from_sse(float(sse), dataset.val_color.numel()), lr))
        lr = ffn.utils.learning_rate_at(1e-3, step, 0.1, 2500)
        losses.append(engine.step(dataset.train_uv3, dataset.train_color_flat, lr))
    model = model.cpu()
    state = {k: v.detach().numpy() for k, v in model.state_dict().items()}
    return np.array([float(x) for x in losses]), reports, state


@pytest.mark.parametrize("name", ["mlp", "positional", "gaussian"])
def test_replays_the_reference_image_regression(name):
    """The reference's own train_image_regression run (64 x 64 synthetic image, 40 steps, reports
    every 10; tests/golden/image_regression.npz) replayed from its initial state with
    RegressionEngine.  The reference computes the loss against float64 targets on the CPU, so
    every step differs in the last bits; Adam keeps those differences relative.  Tolerances
    measured once on an MI355X, worst over the three models in brackets: losses 1e-4 relative
    [2.6e-5], PSNR 0.01 dB at every report [4.6e-5 dB], final weights 1e-2 absolute [4.2e-3,
    positional]: Adam divides by sqrt(v), so a weight whose gradients stay near zero moves by up to
    lr per step whatever their last bits are (40 steps x 1e-3)."""
    g = np.load(os.path.join(GOLDEN, "image_regression.npz"))
    losses, reports, state = _replay(g, name)
    ref_loss = g[name + "/loss"]
    assert len(losses) == len(ref_loss) == int(g["num_steps"]) + 1
    worst = {"loss_rel": float(np.max(np.abs(losses / ref_loss - 1))),
             "psnr": float(np.max(np.abs(np.array([r[1] for r in reports]) - g[name + "/report_psnr"]))),
             "state": max(float(np.max(np.abs(state[k[len(name) + 7:]] - g[k])))
                          for k in g.files if k.startswith(name + "/final/"))}
    print("image regression replay %s worst deviations %s" % (name, worst))
    assert [r[0] for r in reports] == g[name + "/report_step"].tolist()
    np.testing.assert_allclose([r[2] for r in reports], g[name + "/report_lr"], rtol=1e-12)
    np.testing.assert_allclose(losses, ref_loss, rtol=1e-4, atol=0)
    np.testing.assert_allclose([r[1] for r in reports], g[name + "/report_psnr"], rtol=0, atol=0.01)
    for key in g.files:
        if key.startswith(name + "/final/"):
            np.testing.assert_allclose(state[key[len(name) + 7:]], g[key], rtol=0, atol=1e-2)


# ----------------------------------------------------------------------------------- driver script
def test_train_image_regression_script(tmp_path):
    """scripts/train_image_regression.py on a small PNG: val PNGs, superres.png and model.pt are
    written, the stdout report lines have the reference's format, and load_model gives back a
    2-input model whose render equals superres.png."""
    from PIL import Image
    from tests.golden.make_image_regression import synthetic_image
    png = str(tmp_path / "img.png")
    Image.fromarray(synthetic_image(40, 48)).save(png)
    out = str(tmp_path / "run")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train_image_regression.py"),
                          png, "positional", out, "--image-size", "32", "--num-steps", "5",
                          "--report-interval", "2", "--num-channels", "32", "--embedding_size", "32",
                          "--make-video"],
                         capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("step ")]
    assert [int(ln.split()[1]) for ln in lines] == [0, 2, 4, 5]
    for ln in lines:
        assert re.fullmatch(r"step \d+ val: -?\d+\.\d+(e-?\d+)? lr: \d\.\d+(e-?\d+)?", ln), ln
    assert lines[0].endswith("lr: 0.001")
    assert "make-video" in res.stderr
    files = set(os.listdir(out))
    assert {"val00000.png", "val00002.png", "val00004.png", "val00005.png", "superres.png", "model.pt"} <= files
    val = np.asarray(Image.open(os.path.join(out, "val00005.png")))
    assert val.shape == (32, 64, 3)
    model = ffn.load_model(os.path.join(out, "model.pt"))
    assert isinstance(model, ffn.FourierFeatureMLP) and model.num_inputs == 2
    model = model.to(dev())
    uv3 = torch.nn.functional.pad(ffn.PixelDataset.generate_uvs(64, dev()).reshape(-1, 2), (0, 1)).contiguous()
    _, image = ffn.RegressionEngine(model).evaluate(uv3, None, want_image=True)
    superres = np.asarray(Image.open(os.path.join(out, "superres.png")))
    assert np.array_equal(image.reshape(64, 64, 3).cpu().numpy(), superres)
