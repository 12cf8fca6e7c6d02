"""Microbenchmark of 2-D image regression at the reference's defaults (train_image_regression.py:
512 x 512 image -> 65 536 training pixels, 3 x 256 channels; positional with embedding 256 -> 512
features, gaussian with sigma 10 and 512 features, and the plain mlp).

Reports per model: the HIP-event time of RegressionEngine.step after warmup, the validation pass
(262 144 pixels: forward + K11 evaluation + u8 frame), achieved TFLOP/s of the step against the
157.3 TF f32-MFMA peak, and -- labelled as a baseline only -- the same loop in plain PyTorch-ROCm
(nn.Linear chain, torch.sigmoid, 0.5 * MSE, autograd, torch.optim.Adam) on the same GPU.

    python scripts/microbench_image_regression.py --steps 50 --warmup 10 [--out result.json]
"""

import argparse
import json
import math
import os
import sys

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fourier_feature_nets_amd as ffn  # noqa: E402

PEAK_TFLOPS = 157.3


def build(name, channels, embedding):
    if name == "mlp":
        return ffn.MLP(2, 3, num_channels=channels)
    if name == "positional":
        return ffn.PositionalFourierMLP(2, 3, 6, num_channels=channels, embedding_size=embedding)
    return ffn.GaussianFourierMLP(2, 3, 10.0, num_channels=channels, embedding_size=embedding)


def step_flops(model, n):
    """Dense-layer FLOPs of one step: forward 2 in out, weight gradient 2 in out, backward data
    2 in out for every layer but the first (per sample)."""
    layers = [(layer.in_features, layer.out_features) for layer in model.layers]
    fwd = sum(2 * i * o for i, o in layers)
    dgrad = sum(2 * i * o for i, o in layers[1:])
    return n * (2 * fwd + dgrad)


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / steps


class TorchBaseline(nn.Module):
    """The reference's FourierFeatureMLP forward (fourier_feature_models.py:57-78) restated in
    plain PyTorch, with the same weights: a baseline only."""

    def __init__(self, model):
        super().__init__()
        self.b = None if model.b_values is None else model.b_values.data.clone()
        self.a = None if model.a_values is None else model.a_values.data.clone()
        self.layers = nn.ModuleList()
        for layer in model.layers:
            lin = nn.Linear(layer.in_features, layer.out_features).to(layer.weight.device)
            lin.weight.data.copy_(layer.weight.data)
            lin.bias.data.copy_(layer.bias.data)
            self.layers.append(lin)

    def forward(self, x):
        if self.b is not None:
            enc = (math.pi * x) @ self.b
            x = torch.cat([self.a * enc.cos(), self.a * enc.sin()], -1)
        for layer in self.layers[:-1]:
            x = torch.relu(layer(x))
        return self.layers[-1](x)


def run(name, args, dev):
    torch.manual_seed(0)
    rng = np.random.RandomState(0)
    image = rng.randint(0, 256, (args.image_size, args.image_size, 3)).astype(np.uint8)
    dataset = ffn.PixelDataset.from_array(image, "RGB", args.image_size).to(dev)
    model = build(name, args.num_channels, args.embedding_size).to(dev)
    baseline = TorchBaseline(model)
    engine = ffn.RegressionEngine(model)
    uv3, target = dataset.train_uv3, dataset.train_color_flat
    n = uv3.shape[0]
    step_ms = timed(lambda: engine.step(uv3, target, 1e-3), args.steps, args.warmup)
    val_ms = timed(lambda: engine.evaluate(dataset.val_uv3, dataset.val_color_flat, want_image=True),
                   max(1, args.steps // 5), 2)
    flops = step_flops(model, n)
    res = {"model": name, "pixels": n, "channels": args.num_channels,
           "features": model.layers[0].in_features, "step_ms": round(step_ms, 4),
           "validation_ms": round(val_ms, 4), "step_gflop": round(flops / 1e9, 2),
           "step_tflops": round(flops / step_ms / 1e9, 2),
           "fraction_of_f32_mfma_peak": round(flops / step_ms / 1e9 / PEAK_TFLOPS, 3)}
    if args.no_baseline:
        return res
    # baseline: train_image_regression.py:179-186 in plain PyTorch on the same GPU
    optim = torch.optim.Adam(baseline.parameters(), 1e-3)
    uv, color = dataset.train_uv, dataset.train_color

    def torch_step():
        optim.zero_grad()
        out = torch.sigmoid(baseline(uv))
        loss = 0.5 * torch.square(out - color).mean()
        loss.backward()
        optim.step()

    torch_ms = timed(torch_step, args.steps, args.warmup)
    res.update(baseline_pytorch_step_ms=round(torch_ms, 4),
               speedup_vs_pytorch_baseline=round(torch_ms / step_ms, 2))
    return res


def main():
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("--steps", type=int, default=50)
    parser.add_argument("--warmup", type=int, default=10)
    parser.add_argument("--image-size", type=int, default=512)
    parser.add_argument("--num-channels", type=int, default=256)
    parser.add_argument("--embedding-size", type=int, default=256)
    parser.add_argument("--models", default="mlp,positional,gaussian")
    parser.add_argument("--no-baseline", action="store_true",
                        help="skip the PyTorch baseline (kernel profiles of the engine alone)")
    parser.add_argument("--out", help="write the results as JSON here")
    args = parser.parse_args()
    dev = torch.device("cuda:0")
    results = []
    for name in args.models.split(","):
        res = run(name, args, dev)
        print(json.dumps(res), flush=True)
        results.append(res)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
