"""Microbenchmark of K29, the per-ray distortion prior of the octree fits.  Recorded, nothing asserted,
nothing tuned afterwards; one seed.

* cost: on the depth-8 and depth-10 density trees of ``scripts/microbench_octree_fit.py`` (the voxel
  radiance field with an opaque ball, 400x400 rays of scene16's training cameras), every ray of
  camera 0 and a shuffled 4096-ray batch, device time (events, best of ``--repeats`` after a warm-up)
  in one process: the backward without the term (``dist_scale = 0``, the entry point of before) and
  with it (K29b), ``octree_distortion`` (K29a) next to ``render_volume`` (K15) and ``leaf_weights``
  (K21a); then whole ``fit_octree`` / ``fit_octree_sh`` steps (wall time of a fit divided by its
  steps) with ``dist_weight`` 0 and 1e-2.  The SH tree is the density tree with its colours in band 0
  of degree 2.
* the experiment, K23's protocol (``scripts/microbench_octree_photo.py``): the procedural torus,
  depth 8, 116 training cameras and 4 held out, every pixel of theirs against the ground-truth
  frame, the point carve and the box carve coloured by ``color_from_images``.  Per carve and per
  ``dist_weight`` in 0, 1e-3, 1e-2, 1e-1: 300 ``fit_octree`` steps at the defaults, then the held-out
  PSNR, the final training loss, the mean ``D`` over the held-out rays before and after, and the
  number of leaves with ``leaf_weights_over < 1e-2`` (what a refine would drop); and the same four
  arms through ``fit_octree_adaptive(rounds=1)``.

The result file is rewritten after every arm, so a run that is cut short leaves what it measured.

    python scripts/microbench_octree_dist.py [--repeats 5] [--out result.json]
"""

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import fourier_feature_nets_amd as ffn  # noqa: E402
from fourier_feature_nets_amd import octree_fit, ops  # noqa: E402
from scripts.microbench_octree_carve import (FIT_STEPS, HELD_OUT, psnr_all_pixels, quiet,  # noqa: E402
                                             torus_dataset)
from scripts.microbench_octree_fit import ModelTargets  # noqa: E402
from scripts.microbench_octree_render import SAMPLES, SIDE, device_ms  # noqa: E402
from scripts.microbench_octree_walk import SCENE, make_sampler, opaque_ball  # noqa: E402

DEFAULT_OUT = os.path.join(ROOT, "profiles", "r27_octree_dist_microbench.json")
WEIGHTS = (0.0, 1e-3, 1e-2, 1e-1)
# hipcc -Rpass-analysis=kernel-resource-usage, gfx950: the modes without and with the term
RESOURCES = {"kGrad": {"vgprs": 61, "occupancy": 8}, "kGradDist": {"vgprs": 74, "occupancy": 6},
             "kGradSH1": {"vgprs": 64, "occupancy": 7}, "kGradSH1Dist": {"vgprs": 80, "occupancy": 6},
             "kGradSH2": {"vgprs": 82, "occupancy": 5}, "kGradSH2Dist": {"vgprs": 91, "occupancy": 5},
             "kLeafWeight": {"vgprs": 39, "occupancy": 8}, "kDistortion": {"vgprs": 47, "occupancy": 8}}


def band0_tree(tree, degree=2):
    """The density tree as an SH tree: its colours in band 0 (logit / Y_0), higher bands zero."""
    data = np.asarray(tree.leaf_data())
    channels = ops.octree_sh_channels(degree)
    basis = (channels - 1) // 3
    rgb = np.clip(data[:, :3].astype(np.float64), 1e-4, 1 - 1e-4)
    rows = np.zeros((len(data), channels), np.float32)
    rows[:, 0:3 * basis:basis] = (np.log(rgb / (1 - rgb)) / 0.28209479177387814).astype(np.float32)
    rows[:, -1] = data[:, 3]
    state = tree.state_dict
    out = ffn.OcTree(state["scale"], state["node_index"], state["leaf_index"], rows, degree)
    out._center = tree.center
    return out


def fit_step_ms(fit, tree, targets, steps, **kwargs):
    fit(tree, targets, None, 4096, num_steps=3, verbose=False, **kwargs)      # warm-up
    torch.cuda.synchronize()
    start = time.perf_counter()
    fit(tree, targets, None, 4096, num_steps=steps, verbose=False, **kwargs)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - start) / steps


def cost(results, write, args):
    scene = dict(np.load(SCENE))
    model = opaque_ball()
    caster = ffn.Raycaster(model)
    fit_cameras = list(range(min(args.fit_cameras, int(scene["split_counts"][0]) - 2)))
    train = ModelTargets(caster, make_sampler(scene, fit_cameras, SIDE, SAMPLES))
    sampler = train.sampler
    per = sampler.rays_per_camera
    out = {"model": "Voxels(64), opaque ball r=0.45", "frame": [SIDE, SIDE],
           "fit_cameras": fit_cameras, "resources": RESOURCES, "cases": []}
    results["cost"] = out
    for depth in args.depths:
        tree = ffn.OcTree.build_from_model(model, depth, alpha_threshold=0.01)
        shift = torch.tensor(tree.center, dtype=torch.float32, device="cuda")
        geometry = (tree.scale, tree.depth, tree._on_device("node_index"),
                    tree._on_device("leaf_index"))
        data = tree._colors_on_device()
        case = {"depth": depth, "leaves": tree.num_leaves, "rays": {}}
        shuffled = torch.randperm(len(sampler), device="cuda",
                                  generator=torch.Generator(device="cuda").manual_seed(2))[:4096]
        for name, rays in (("camera_0", torch.arange(per, device="cuda")),
                           ("batch_4096", shuffled)):
            o = (sampler.starts[rays] - shift).contiguous()
            d = sampler.directions[rays].contiguous()
            count = int(rays.numel())
            g = torch.randn((count, 3), device="cuda") * 1e-4
            ga = torch.randn((count,), device="cuda") * 1e-4
            ray_d = torch.empty((count,), dtype=torch.float32, device="cuda")
            weights = torch.zeros((tree.num_leaves,), dtype=torch.float32, device="cuda")
            space = ops.OctreeGradWorkspace()
            old = lambda: ops.octree_render_volume_backward(  # noqa: E731
                o, d, *geometry, data, g, ga, workspace=space)
            new = lambda: ops.octree_render_volume_backward(  # noqa: E731
                o, d, *geometry, data, g, ga, workspace=space, dist_scale=1e-2 / count,
                ray_distortion=ray_d)
            new()                                       # sizes the workspace for both
            old_ms, new_ms = device_ms(old, args.repeats), device_ms(new, args.repeats)
            render_ms = device_ms(lambda: ops.octree_render_volume(o, d, *geometry, data),
                                  args.repeats)
            weights_ms = device_ms(lambda: ops.octree_leaf_weights(o, d, *geometry, data, 4, 3,
                                                                   out=weights), args.repeats)
            dist_ms = device_ms(lambda: ops.octree_distortion(o, d, *geometry, data, 4, 3),
                                args.repeats)
            case["rays"][name] = {
                "rays": count, "entries": space.entries,
                "mean_distortion": float(ray_d.mean().item()),
                "backward_without_term_device_ms": old_ms, "backward_with_term_device_ms": new_ms,
                "with_over_without": new_ms / old_ms,
                "render_volume_device_ms": render_ms,
                "leaf_weights_folding_device_ms": weights_ms, "distortion_k29a_device_ms": dist_ms,
                "k29a_over_render_volume": dist_ms / render_ms,
                "k29a_over_leaf_weights": dist_ms / weights_ms}
            print(json.dumps({name: case["rays"][name]}), flush=True)
        wide = band0_tree(tree)
        case["fit_step_wall_ms"] = {
            "steps": args.steps,
            "fit_octree_dist_weight_0": fit_step_ms(ffn.fit_octree, tree, train, args.steps),
            "fit_octree_dist_weight_1e-2": fit_step_ms(ffn.fit_octree, tree, train, args.steps,
                                                       dist_weight=1e-2),
            "fit_octree_sh_degree_2_dist_weight_0": fit_step_ms(ffn.fit_octree_sh, wide, train,
                                                                args.steps),
            "fit_octree_sh_degree_2_dist_weight_1e-2": fit_step_ms(ffn.fit_octree_sh, wide, train,
                                                                   args.steps, dist_weight=1e-2)}
        print(json.dumps(case["fit_step_wall_ms"]), flush=True)
        out["cases"].append(case)
        write()
        del tree, wide, data
        torch.cuda.empty_cache()


def mean_distortion(tree, dataset, center):
    sampler = dataset.sampler
    shift = torch.tensor(center, dtype=torch.float32, device=sampler.starts.device)
    per = sampler.rays_per_camera
    total = 0.0
    for camera in range(sampler.num_cameras):
        rays = slice(camera * per, (camera + 1) * per)
        d = tree.distortion((sampler.starts[rays] - shift).contiguous(),
                            sampler.directions[rays].contiguous())
        total += float(d.sum(dtype=torch.float64).item())
    return total / (per * sampler.num_cameras)


def experiment(results, write, args):
    num_cameras = args.cameras
    truth, images, cameras, bounds = torus_dataset(num_cameras, args.size, args.truth_depth)
    center, scale = truth.center, truth.scale
    train_n = num_cameras - HELD_OUT
    train = quiet(ffn.ImageDataset, "train", images[:train_n], bounds, cameras[:train_n], 8,
                  device="cuda")
    held = quiet(ffn.ImageDataset, "val", images[train_n:], bounds, cameras[train_n:], 8,
                 device="cuda")

    def psnr(tree):
        return psnr_all_pixels(lambda starts, dirs: tree.render_volume(starts, dirs).color, held,
                               center)

    def scored(tree, log):
        weights = octree_fit.leaf_weights_over(tree, train, center)
        return {"leaves": tree.num_leaves, "held_out_psnr": psnr(tree),
                "final_training_loss": log[-1].loss,
                "training_loss_last_16": float(np.mean([e.loss for e in log[-16:]])),
                "held_out_mean_distortion": mean_distortion(tree, held, center),
                "leaves_with_weight_below_1e-2": int((weights < 1e-2).sum()),
                "share_of_leaves_with_weight_below_1e-2": float((weights < 1e-2).mean())}

    out = {"dataset": "procedural_torus() at depth %d, %d cameras of %d x %d, first-hit frames"
                      % (args.truth_depth, num_cameras, args.size, args.size),
           "depth": args.fit_depth, "train_cameras": train_n, "held_out_cameras": HELD_OUT,
           "fit_steps": FIT_STEPS, "seed": "fit_octree's default, one seed",
           "earlier_figures_without_the_term": {"point": 27.13, "box": 23.38}, "arms": []}
    results["experiment"] = out
    for footprint in ("point", "box"):
        hull = ffn.OcTree.build_from_silhouettes(train, args.fit_depth, center, scale,
                                                 footprint=footprint)
        tree = hull.color_from_images(train, center)[0]
        before = {"leaves": tree.num_leaves, "held_out_psnr": psnr(tree),
                  "held_out_mean_distortion": mean_distortion(tree, held, center)}
        for weight in WEIGHTS:
            arm = {"carve": footprint, "dist_weight": weight, "as_built": before}
            kwargs = {} if weight == 0.0 else {"dist_weight": weight}
            torch.cuda.synchronize()
            start = time.perf_counter()
            fitted, log = ffn.fit_octree(tree, train, None, num_steps=FIT_STEPS, verbose=False,
                                         **kwargs)
            torch.cuda.synchronize()
            arm["fit_octree_step_wall_ms"] = 1e3 * (time.perf_counter() - start) / FIT_STEPS
            arm["fit_octree"] = scored(fitted, log)
            print(json.dumps(arm), flush=True)
            write()
            refined, logs, reports = ffn.fit_octree_adaptive(tree, train, None, rounds=1,
                                                             num_steps=FIT_STEPS, verbose=False,
                                                             **kwargs)
            arm["fit_octree_adaptive_rounds_1"] = dict(scored(refined, logs[-1]),
                                                       report=reports[0]._asdict())
            out["arms"].append(arm)
            print(json.dumps(arm["fit_octree_adaptive_rounds_1"]), flush=True)
            del fitted, refined
            torch.cuda.empty_cache()
            write()


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--repeats", type=int, default=5)
    parser.add_argument("--depths", type=int, nargs="*", default=[8, 10])
    parser.add_argument("--fit-cameras", type=int, default=8)
    parser.add_argument("--steps", type=int, default=40, help="steps of the timed fits")
    parser.add_argument("--cameras", type=int, default=120)
    parser.add_argument("--size", type=int, default=400)
    parser.add_argument("--truth-depth", type=int, default=9)
    parser.add_argument("--fit-depth", type=int, default=8)
    parser.add_argument("--skip-cost", action="store_true")
    parser.add_argument("--skip-experiment", action="store_true")
    parser.add_argument("--out", default=DEFAULT_OUT)
    args = parser.parse_args()
    results = {}
    if os.path.exists(args.out) and (args.skip_cost or args.skip_experiment):
        with open(args.out) as f:                       # the other half, measured earlier
            results = json.load(f)
    results.update({
        "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
        "precision": "f32 (no matrix work on this path; bf16x6 not run)",
        "not_measured": "rocprofv3 kernel times; other scenes; SH trees in the experiment; "
                        "seed-to-seed spread (one seed)"})

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(results, indent=1) + "\n")

    if not args.skip_cost:
        cost(results, write, args)
    if not args.skip_experiment:
        experiment(results, write, args)
    write()
    return 0


if __name__ == "__main__":
    sys.exit(main())
