"""Microbenchmark of K26 (``OcTree.focus_samples`` / ``RaySampler.focus_on_octree``): focus samples
drawn from an octree's own weights, and the experiment it exists for.

The dataset is the one ``scripts/make_mesh_npz.py`` writes for the procedural torus, made in memory
(``microbench_octree_carve.torus_dataset``: 120 cameras of 400 x 400, the last 4 held out).  The trees
are carved from the 116 training cameras at depth 8 and depth 10 (K23, ``color="visible"``, no fit).
Recorded, nothing asserted, nothing tuned afterwards; events, best of ``--repeats`` after a warm-up:

* per tree, on a shuffled 4096-ray batch and on one camera's 160 000 rays, S = 128 (64 uniform + 64
  focus): K26 alone, K2a + K26 (``sample_t`` of the tree-focused sampler), and ``render_volume`` on
  the same rays in the same process -- the walk without emits, so that K26's two walks plus the emits
  stand against one; the share of the rays with mass >= min_mass;
* in the same process the live coarse pass of the tiny NeRF on the same rays: ``sample_t`` of a
  sampler whose opacity model is an (untrained: the time does not depend on the weights) tiny NeRF,
  focus_mode "live" (K2a + ``MlpProgram.focus_sample``);
* the experiment: the tiny NeRF of ``train_tiny_nerf.py`` at its defaults (positional, 256 channels,
  128 samples, batch 1024, lr 5e-4, anneal and crop schedule as the driver's) for ``--steps`` steps
  on the 116 cameras, three arms from ONE seed -- (a) stratified uniform, (b) focus samples from the
  depth-8 carved tree, (c) from the same tree after 300 ``fit_octree`` steps -- held-out PSNR (every
  pixel of the 4 cameras, black background) and ms per step.  One seed: the spread is not measured.

    python scripts/microbench_octree_focus.py [--repeats 5] [--steps 2000] [--out result.json]
"""

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fourier_feature_nets_amd as ffn  # noqa: E402
from scripts.microbench_octree_carve import HELD_OUT, quiet, torus_dataset  # noqa: E402
from scripts.microbench_octree_render import device_ms  # noqa: E402

DEFAULT_OUT = os.path.join(ROOT, "profiles", "r24_octree_focus_microbench.json")
SAMPLES = 128
FIT_STEPS = 300


def kernel_cases(tree, center, sampler, live, batches, repeats):
    focused = sampler.focus_on_octree(tree, center)
    shift = torch.tensor(center, dtype=torch.float32, device=sampler.device)
    n_uniform = SAMPLES // 2
    n_focus = SAMPLES - n_uniform
    out = []
    for name, index in batches:
        rows = index.shape[0]
        half = ffn.ops.sample_t(sampler.near_far, index, n_uniform, sampler._unit(n_uniform), None,
                                None)
        u = sampler._unit(n_focus).unsqueeze(0).repeat(rows, 1).contiguous()
        starts = (sampler.starts[index] - shift).contiguous()
        dirs = sampler.directions[index].contiguous()
        mass = focused.focus_mass(index)
        case = {"rays": name, "count": rows, "samples": SAMPLES,
                "share_with_mass": float((mass >= focused.focus_min_mass).float().mean()),
                "k26_ms": device_ms(lambda: tree.focus_samples(
                    sampler.starts, sampler.directions, sampler.near_far, index, u, half, center),
                    repeats),
                "k2a_plus_k26_sample_t_ms": device_ms(lambda: focused.sample_t(index, None), repeats),
                "render_volume_ms": device_ms(lambda: tree.render_volume(starts, dirs), repeats),
                "live_coarse_sample_t_ms": device_ms(lambda: live.sample_t(index, None), repeats)}
        out.append(case)
        print(json.dumps(case), flush=True)
    return out


def held_out_psnr(caster, held):
    sampler = held.sampler
    per = sampler.rays_per_camera
    error = 0.0
    with torch.no_grad():
        for camera in range(sampler.num_cameras):
            first = camera * per
            index = torch.arange(first, first + per, dtype=torch.int64, device=sampler.device)
            color = torch.zeros((per, 3), dtype=torch.float32, device=sampler.device)
            keep = sampler.valid_index(index)
            for b0 in range(0, keep.numel(), 1 << 15):
                rays = keep[b0:b0 + (1 << 15)].contiguous()
                out = caster.render_rays(sampler, rays)
                color[rays - first] = out.color
            error += float(((color - held.colors[index]) ** 2).sum(dtype=torch.float64).item())
    return float(-10 * np.log10(max(error / (3 * per * sampler.num_cameras), 1e-12)))


def train_arm(name, images, cameras, bounds, tree, center, steps, seed):
    train_n = len(cameras) - HELD_OUT
    torch.manual_seed(seed)
    torch.cuda.manual_seed(seed)
    np.random.seed(seed)
    model = ffn.PositionalFourierMLP(3, 4, max_log_scale=5.5, embedding_size=256,
                                     num_channels=256).to("cuda")
    train = quiet(ffn.ImageDataset, "train", images[:train_n], bounds, cameras[:train_n], SAMPLES,
                  True, True, None, 1024, "RGB", anneal_start=0.2, num_anneal_steps=2000,
                  device="cuda")
    held = quiet(ffn.ImageDataset, "val", images[train_n:], bounds, cameras[train_n:], SAMPLES,
                 True, False, None, 1024, "RGB", device="cuda")
    if tree is not None:
        train.sampler = train.sampler.focus_on_octree(tree, center)
        held.sampler = held.sampler.focus_on_octree(tree, center)
    caster = ffn.Raycaster(model)
    # the driver's report interval: the centre crop is lifted at the report of step 1000
    log = quiet(caster.fit, train, held, 1024, 5e-4, steps, 1000, 1000, 0.1, 25000, 0.0, [])
    # wall time per step between the last two reports (full frames; one validation pass included)
    last, before = log[-1], log[-2]
    arm = {"arm": name, "steps": steps,
           "ms_per_step_wall_between_the_last_two_reports":
           1000.0 * (last.timestamp - before.timestamp) / (last.step - before.step),
           "fit_log_val_psnr": [float(e.val_psnr) for e in log],
           "held_out_psnr_all_pixels": held_out_psnr(caster, held)}
    print(json.dumps(arm), flush=True)
    return arm


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--repeats", type=int, default=5)
    parser.add_argument("--depths", type=int, nargs="+", default=[8, 10])
    parser.add_argument("--size", type=int, default=400)
    parser.add_argument("--num-cameras", type=int, default=120)
    parser.add_argument("--truth-depth", type=int, default=9)
    parser.add_argument("--steps", type=int, default=2000)
    parser.add_argument("--seed", type=int, default=20080524)
    parser.add_argument("--skip-experiment", action="store_true")
    parser.add_argument("--out", default=DEFAULT_OUT)
    args = parser.parse_args()
    truth, images, cameras, bounds = torus_dataset(args.num_cameras, args.size, args.truth_depth)
    center, scale = truth.center, truth.scale
    train_n = args.num_cameras - HELD_OUT
    results = {"device": torch.cuda.get_device_name(0),
               "dataset": "procedural_torus() at depth %d, %d cameras of %d x %d (the last %d held "
                          "out), first-hit frames" % (args.truth_depth, args.num_cameras, args.size,
                                                      args.size, HELD_OUT),
               "cube": {"center": list(center), "scale": scale}, "repeats": args.repeats,
               "timing": "events around the call, best of repeats after one warm-up",
               "not_measured": "rocprofv3 kernel times; --precision bf16x6; the spread over seeds",
               "min_mass": 1e-3, "trees": []}
    train = quiet(ffn.ImageDataset, "train", images[:train_n], bounds, cameras[:train_n], SAMPLES,
                  device="cuda")
    sampler = train.sampler
    coarse = ffn.PositionalFourierMLP(3, 4, max_log_scale=5.5, embedding_size=256,
                                      num_channels=256).to("cuda")
    live = quiet(ffn.RaySampler, bounds, cameras[:train_n], SAMPLES, False, coarse, device="cuda",
                 focus_mode="live")
    generator = torch.Generator().manual_seed(1)
    valid = sampler.valid_index(torch.arange(len(sampler), device=sampler.device))
    shuffled = valid[torch.randperm(valid.numel(), generator=generator)[:4096].to(valid.device)]
    per = sampler.rays_per_camera
    one_camera = torch.arange(0, per, dtype=torch.int64, device=sampler.device)
    batches = [("shuffled batch", shuffled.contiguous()), ("camera 0, every pixel", one_camera)]
    trees = {}
    for depth in args.depths:
        tree = ffn.OcTree.build_from_silhouettes(train, depth, center, scale, color="visible")
        trees[depth] = tree
        entry = {"depth": depth, "leaves": tree.num_leaves,
                 "cases": kernel_cases(tree, center, sampler, live, batches, args.repeats)}
        results["trees"].append(entry)
        torch.cuda.empty_cache()
    if not args.skip_experiment:
        carved = trees.get(8) or ffn.OcTree.build_from_silhouettes(train, 8, center, scale,
                                                                   color="visible")
        fitted, _ = ffn.fit_octree(carved, train, None, num_steps=FIT_STEPS, verbose=False)
        del train, live
        torch.cuda.empty_cache()
        arms = [("a: stratified uniform", None), ("b: focus on the depth-8 carved tree", carved),
                ("c: the same tree after %d fit_octree steps" % FIT_STEPS, fitted)]
        results["experiment"] = {
            "model": "PositionalFourierMLP(3, 4, max_log_scale 5.5, embedding 256, 256 channels), "
                     "train_tiny_nerf.py defaults: 128 samples, batch 1024, lr 5e-4, crop 1000 "
                     "steps, anneal from 0.2 over 2000 steps, decay 0.1 per 25000",
            "seed": args.seed, "seeds": 1, "spread": "not measured",
            "arms": [train_arm(name, images, cameras, bounds, tree, center, args.steps, args.seed)
                     for name, tree in arms]}
    line = json.dumps(results, indent=1)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
