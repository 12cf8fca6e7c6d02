"""Microbenchmark of 1-D signal regression at the reference's defaults (train_signal_regression.py:
multifreq, 32 training samples x rate 8 -> 256 validation points, 1 x 64 channels, plain and
--fourier with 16 frequencies).

Reports per configuration:
- the HIP-event time of RegressionEngine.step (linear MSE, weight decay 1e-3) after warmup, and
  the C-ABI entry points it calls per step;
- the wall time of the full default run (10 000 steps + 201 validations, --no-plot) of
  scripts/train_signal_regression.py in a fresh process, and the wall time of its training loop
  alone measured in-process;
- labelled as a baseline only, the same loop in eager PyTorch-ROCm on the same GPU (nn.Linear
  chain, MSE, autograd, torch.optim.Adam with weight_decay=1e-3): step time and loop wall time.

    python scripts/microbench_signal_regression.py --steps 2000 --warmup 200 [--out result.json]

Kernel dispatches per step come from a separate profiled run (``--no-baseline --no-full-run``
under ``rocprofv3 --kernel-trace --stats``): total calls / (steps + warmup).
"""

import argparse
import json
import math
import os
import subprocess
import sys
import tempfile
import time

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fourier_feature_nets_amd as ffn  # noqa: E402
from fourier_feature_nets_amd import _lib  # noqa: E402
from scripts import train_signal_regression as driver  # noqa: E402


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
    plain PyTorch with the same weights (0-d output bias included): a baseline only."""

    def __init__(self, model):
        super().__init__()
        self.b = None if model.b_values is None else model.b_values.data.clone()
        self.a = None if model.a_values is None else model.a_values.data.clone()
        self.layers = nn.ModuleList()
        for layer in model.layers:
            lin = nn.Linear(layer.in_features, layer.out_features).to(layer.weight.device)
            lin.weight.data.copy_(layer.weight.data)
            lin.bias.data = layer.bias.data.clone()
            self.layers.append(lin)

    def forward(self, x):
        if self.b is not None:
            enc = (math.pi * x) @ self.b
            x = torch.cat([self.a * enc.cos(), self.a * enc.sin()], -1)
        for layer in self.layers[:-1]:
            x = torch.relu(layer(x))
        return self.layers[-1](x)


class CountCalls:
    """Counts C-ABI entry-point calls (libffn_hip) while active."""

    def __enter__(self):
        self.count = 0
        self._orig = _lib.call

        def call(name, *args):
            self.count += 1
            return self._orig(name, *args)

        _lib.call = call
        return self

    def __exit__(self, *exc):
        _lib.call = self._orig


def loop_wall(step_fn, validate_fn, num_steps):
    """Wall seconds of the driver's loop: num_steps + 1 steps, a validation read back to the host
    at every 50th step and the last (as train_signal_regression.py:153-182 without plotting)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for step in range(num_steps + 1):
        loss = step_fn()
        if step % 50 == 0 or step == num_steps:
            validate_fn()
            loss.item()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def run(fourier, args, dev):
    ns = argparse.Namespace(fourier=fourier, num_samples=32, num_channels=64, num_layers=1)
    dataset = ffn.SignalDataset.create(driver.multifreq, 32, 8)
    torch.manual_seed(0)
    model = driver.build_model(ns, dataset).to(dev)
    baseline = TorchBaseline(model)
    engine = ffn.RegressionEngine(model, weight_decay=driver.WEIGHT_DECAY, loss="linear")
    data = dataset.to(dev)
    x3, y, vx3, vy = data.train_x3, data.train_y, data.val_x3, data.val_y
    step = lambda: engine.step(x3, y, driver.LEARNING_RATE)   # noqa: E731
    step_ms = timed(step, args.steps, args.warmup)
    with CountCalls() as calls:
        step()
    torch.cuda.synchronize()
    res = {"config": "fourier" if fourier else "plain", "train_samples": int(y.shape[0]),
           "val_points": int(vy.shape[0]), "features": model.layers[0].in_features,
           "channels": 64, "step_ms": round(step_ms, 4), "abi_calls_per_step": calls.count}
    if args.no_full_run:
        return res
    res["loop_10000_steps_s"] = round(loop_wall(step, lambda: engine.validation_loss(vx3, vy).item(),
                                                10000), 3)
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "train_signal_regression.py"), "multifreq",
           os.path.join(args.tmp, "run_%s" % res["config"]), "--no-plot"] + (["--fourier"] if fourier else [])
    t0 = time.perf_counter()
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    res["driver_10000_steps_wall_s"] = round(time.perf_counter() - t0, 3)
    if out.returncode != 0:
        raise RuntimeError(out.stderr[-2000:])
    res["driver_final_line"] = out.stdout.strip().splitlines()[-1]
    if args.no_baseline:
        return res
    # baseline: train_signal_regression.py:141,153-157 in eager PyTorch on the same GPU
    optim = torch.optim.Adam(baseline.parameters(), driver.LEARNING_RATE,
                             weight_decay=driver.WEIGHT_DECAY)
    tx, vx = data.train_x, data.val_x

    def torch_step():
        optim.zero_grad()
        loss = (baseline(tx) - y).square().mean()
        loss.backward()
        optim.step()
        return loss

    def torch_validate():
        with torch.no_grad():
            return (baseline(vx) - vy).square().mean().item()

    torch_ms = timed(torch_step, args.steps, args.warmup)
    res.update(baseline_pytorch_step_ms=round(torch_ms, 4),
               baseline_pytorch_loop_10000_steps_s=round(loop_wall(torch_step, torch_validate, 10000), 3),
               speedup_vs_pytorch_baseline=round(torch_ms / step_ms, 2))
    return res


def main():
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("--steps", type=int, default=2000)
    parser.add_argument("--warmup", type=int, default=200)
    parser.add_argument("--configs", default="plain,fourier")
    parser.add_argument("--no-baseline", action="store_true", help="skip the PyTorch baseline")
    parser.add_argument("--no-full-run", action="store_true",
                        help="skip the 10 000-step runs (kernel profiles of the step alone)")
    parser.add_argument("--tmp", default=None,
                        help="results directory of the driver runs (default: a temporary one)")
    parser.add_argument("--out", help="write the results as JSON here")
    args = parser.parse_args()
    if args.tmp is None:
        args.tmp = tempfile.mkdtemp(prefix="signal_microbench_")
    os.makedirs(args.tmp, exist_ok=True)
    dev = torch.device("cuda:0")
    results = []
    for config in args.configs.split(","):
        res = run(config == "fourier", args, dev)
        print(json.dumps(res), flush=True)
        results.append(res)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "steps": args.steps,
                       "warmup": args.warmup, "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
