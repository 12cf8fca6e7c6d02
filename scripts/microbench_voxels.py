"""Timing of voxel training at the train_voxels.py defaults (side 128, 1024 rays x 256 samples):
K10 forward, the K10b backward on the annealed first-step samples (anneal_start 0.2: every ray's
samples squeezed into the middle fifth of its span, many samples per cell) and on full-range
samples, clip+Adam over 4 * 128^3 + 4 parameters, and the whole TrainEngine.train_step.  Baseline,
same GPU and inputs: ATen's grid_sample(padding_mode="border", align_corners=False) backward.
HIP events on the launch stream, warm-up first, median of --iters runs; one JSON line out.

    python scripts/microbench_voxels.py [--iters 30] [--out FILE] [--steps-only K]

--steps-only K runs K train steps and nothing else (for a rocprofv3 --kernel-trace --stats run)."""

import argparse
import contextlib
import io
import json
import os
import subprocess
import sys
import tempfile

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fourier_feature_nets_amd as ffn  # noqa: E402
from fourier_feature_nets_amd import ops  # noqa: E402


def timed(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    times.sort()
    return {"median_us": times[len(times) // 2], "min_us": times[0], "max_us": times[-1], "runs": iters}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=128)
    ap.add_argument("--rays", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps-only", type=int, default=0)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    tmp = tempfile.mkdtemp()
    scene = os.path.join(tmp, "scene.npz")
    subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "make_synthetic_npz.py"), scene,
                    "--size", "128", "--cameras", "24"], check=True, capture_output=True)
    torch.manual_seed(20080524)
    with contextlib.redirect_stdout(io.StringIO()):
        train = ffn.ImageDataset.load(scene, "train", args.samples, True, True, anneal_start=0.2,
                                      num_anneal_steps=2000, device=dev)
    scale = 2 / float(train.sampler.bounds[0, 0])
    side = args.side
    model = ffn.Voxels(side, scale).to(dev)
    engine = ffn.TrainEngine(model)
    batch = torch.randperm(len(train), device=dev)[:args.rays]
    if args.steps_only:
        for step in range(args.steps_only):
            engine.train_step(train, batch, step, 0.01)
        torch.cuda.synchronize()
        return 0
    rays = train.ray_ids(batch)
    sets = {}
    for name, step in (("annealed_step0", 0), ("full_range", 10 ** 6)):
        _, pos, _ = train.sampler.sample_points(rays, step, want_views=False)
        pos = pos.reshape(-1, 3).contiguous()
        sets[name] = (pos, (torch.randn((pos.shape[0], 4), device=dev) / pos.shape[0]).contiguous())
    vol = model.voxels.detach().reshape(4, side, side, side)
    bias = model.bias.detach().reshape(4)
    n = sets["full_range"][0].shape[0]
    ws = torch.empty(((ops.voxels_backward_workspace_bytes(n, side) + 3) // 4,), device=dev)
    d_vol = torch.empty((4, side, side, side), device=dev)
    d_bias = torch.empty((4,), device=dev)
    res = {"what": "voxel training kernels, side %d, %d rays x %d samples (train_voxels defaults)"
           % (side, args.rays, args.samples), "samples": n, "device": torch.cuda.get_device_name(0)}
    pos_full = sets["full_range"][0]
    res["k10_forward"] = timed(lambda: ops.voxels_forward(vol, bias, pos_full, side, scale), args.iters)
    for name, (pos, g) in sets.items():
        cells = (((pos / scale + 1) * side - 1) / 2).clamp(0, side - 1).floor().long()
        lin = (cells[:, 2] * side + cells[:, 1]) * side + cells[:, 0]
        counts = torch.bincount(lin)
        counts = counts[counts > 0].float()
        res["backward_" + name] = timed(
            lambda: ops.voxels_backward(pos, g, side, scale, workspace=ws, d_volume=d_vol, d_bias=d_bias),
            args.iters)
        res["backward_" + name].update(occupied_cells=int(counts.numel()),
                                       median_samples_per_cell=float(counts.median()),
                                       max_samples_per_cell=int(counts.max()))
        # baseline: ATen's autograd backward of grid_sample (float atomics) on the same inputs
        v = model.voxels.detach().clone().requires_grad_(True)
        out = F.grid_sample(v, (pos / scale).reshape(1, -1, 1, 1, 3), padding_mode="border",
                            align_corners=False)
        gout = g.t().reshape(1, 4, -1, 1, 1).contiguous()
        res["aten_grid_sample_backward_" + name] = timed(
            lambda: torch.autograd.grad(out, v, gout, retain_graph=True), args.iters)
    params = torch.zeros((4 * side ** 3 + 4,), device=dev)
    grads = torch.randn_like(params) * 1e-3
    m, v2 = torch.zeros_like(params), torch.zeros_like(params)
    scratch = torch.empty(((params.numel() + 1023) // 1024,), device=dev)
    norm = torch.zeros((1,), device=dev)
    res["clip_adam"] = timed(lambda: ops.clip_adam(params, grads, m, v2, 1, 0.01, scratch=scratch,
                                                   norm_out=norm), args.iters)
    res["clip_adam"]["parameters"] = int(params.numel())
    step = [0]

    def one_step():
        engine.train_step(train, batch, step[0], 0.01)
        step[0] += 1

    res["train_step_annealed"] = timed(one_step, args.iters)
    for name in ("annealed_step0", "full_range"):
        res["backward_beats_aten_" + name] = (res["backward_" + name]["median_us"]
                                              < res["aten_grid_sample_backward_" + name]["median_us"])
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
