"""Microbenchmark of the K20 total-variation prior: the plan, the per-step kernels next to the
backward they are added to, and the held-out experiment of the K17 paragraph with the prior off and on.

The trees are those of ``scripts/microbench_octree_density.py`` and of the K17 / K19 microbenchmarks:
the density trees of the voxel radiance field with an opaque ball (``OcTree.build_from_model``) at
``--depths``, the rays the 400x400 frames of ``tests/golden/scene16.npz``.  In one process, device
time between events, best of ``--repeats`` after a warm-up call, per depth:

* ``L``, ``E`` and the longest incidence list; the wall time of K20a plus the plan
  (``ops.octree_neighbors`` + ``ops.octree_tv_plan``, synchronised), best of ``--repeats``;
* K20b + K20c (``ops.octree_tv`` with ``accumulate``) on the plain tree's rows and on the rows of
  ``bake_sh`` at degree 2;
* K17a + K17b and K19a + K19b on a 4096-ray batch of the same tree, and one whole fit step
  (``fit_octree`` / ``fit_octree_sh``: mean wall time of ``--steps`` steps inside a longer run) with
  the prior off and on.

The held-out experiment, on the first depth: the tree is fitted to the model's own renders of the
training cameras for ``--fit-steps`` steps at ``--learning-rates``, with ``tv_weight`` off and at
``--tv-weights`` (the same number for colour and density), and the PSNR against the model's render of
two held-out cameras is recorded over all pixels and where the model is opaque.  Nothing here
asserts a time or a PSNR, and nothing is tuned after the result.  Kernel times under rocprofv3 are
not collected.

The result is written after every section, so that a run that is cut short leaves what it had.

    python scripts/microbench_octree_tv.py [--repeats 5] [--out profiles/r18_octree_tv_microbench.json]

``--out`` defaults to ``profiles/r18_octree_tv_microbench.json``, the recorded run.
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
import fourier_feature_nets_amd as ffn  # noqa: E402
from fourier_feature_nets_amd import ops  # noqa: E402
from scripts.microbench_octree_fit import ModelTargets, psnr_pair  # noqa: E402
from scripts.microbench_octree_render import SAMPLES, SIDE, device_ms  # noqa: E402
from scripts.microbench_octree_walk import SCENE, make_sampler, opaque_ball  # noqa: E402


def plan_wall_ms(tree, repeats):
    nodes, leaves = tree._on_device("node_index"), tree._on_device("leaf_index")
    best = float("inf")
    for _ in range(repeats + 1):
        torch.cuda.synchronize()
        begin = time.perf_counter()
        plan = ops.octree_tv_plan(ops.octree_neighbors(nodes, leaves), leaves)
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - begin) * 1e3)
        del plan
    return best


def tv_ms(rows, plan, lam, repeats):
    grads = torch.zeros_like(rows)
    both = device_ms(lambda: ops.octree_tv(rows, plan, lam, 1e-2, grads, True), repeats)
    return {"k20b_k20c_accumulate_device_ms": both,
            "workspace_bytes": int(plan.workspace(rows.shape[1]).numel()) * 4}


def step_wall_ms(fit, tree, train, steps, **prior):
    """Mean wall ms of a step: a run of ``steps + 4`` steps minus a run of 4, over ``steps``."""
    def run(count):
        torch.cuda.synchronize()
        begin = time.perf_counter()
        fit(tree, train, None, 4096, num_steps=count, verbose=False, **prior)
        torch.cuda.synchronize()
        return (time.perf_counter() - begin) * 1e3
    run(4)                                              # warm-up: workspaces, the plan
    short = min(run(4) for _ in range(2))
    return (min(run(steps + 4) for _ in range(2)) - short) / steps


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--repeats", type=int, default=5)
    parser.add_argument("--steps", type=int, default=20)
    parser.add_argument("--depths", type=int, nargs="+", default=[8, 10])
    parser.add_argument("--num-views", type=int, default=64)
    parser.add_argument("--fit-cameras", type=int, default=8)
    parser.add_argument("--fit-steps", type=int, default=300)
    parser.add_argument("--learning-rates", type=float, nargs="+", default=[1e-3, 1e-2])
    parser.add_argument("--tv-weights", type=float, nargs="+", default=[1e-4, 1e-3])
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles",
                                                      "r18_octree_tv_microbench.json"))
    args = parser.parse_args()

    def write(results):
        line = json.dumps(results, indent=1)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(line + "\n")
        return line

    scene = dict(np.load(SCENE))
    n_train = int(scene["split_counts"][0])
    model = opaque_ball()
    caster = ffn.Raycaster(model)
    fit_cameras = list(range(min(args.fit_cameras, n_train - 2)))
    held_out = [n_train - 2, n_train - 1]
    train = ModelTargets(caster, make_sampler(scene, fit_cameras, SIDE, SAMPLES))
    val = ModelTargets(caster, make_sampler(scene, held_out, SIDE, SAMPLES))
    sampler = train.sampler
    results = {"device": torch.cuda.get_device_name(0), "model": "Voxels(64), opaque ball r=0.45",
               "precision": "f32 (no matrix work on this path; bf16x6 not run)",
               "rocprofv3_kernel_times": "not collected", "frame": [SIDE, SIDE],
               "repeats": args.repeats, "tv_eps": 1e-2,
               "targets": "the model's own render (colour * alpha, alpha)",
               "fit_cameras": fit_cameras, "held_out_cameras": held_out, "cases": [],
               "complete": False}
    for depth in args.depths:
        tree = ffn.OcTree.build_from_model(model, depth, alpha_threshold=0.01)
        plan = tree._tv_plan()
        case = {"depth": depth, "leaves": tree.num_leaves, "edges": plan.num_edges,
                "longest_incidence_list": plan.longest,
                "neighbors_and_plan_wall_ms": plan_wall_ms(tree, args.repeats)}
        results["cases"].append(case)
        write(results)
        rows = tree._colors_on_device()
        case["plain_stride_4"] = tv_ms(rows, plan, ops.octree_tv_weights(None, 4), args.repeats)
        sh_tree = tree.bake_sh(model, 2, args.num_views)
        sh_rows = sh_tree._sh_rows_on_device()
        case["sh_degree_2_stride_28"] = tv_ms(sh_rows, plan, ops.octree_tv_weights(None, 28, 2),
                                              args.repeats)
        write(results)
        # the backwards the prior is added to, on a 4096-ray batch
        shift = torch.tensor(tree.center, dtype=torch.float32, device="cuda")
        rays = torch.randperm(len(sampler), device="cuda",
                              generator=torch.Generator(device="cuda").manual_seed(2))[:4096]
        o = (sampler.starts[rays] - shift).contiguous()
        d = sampler.directions[rays].contiguous()
        g = torch.randn((4096, 3), device="cuda") * 1e-4
        ga = torch.randn((4096,), device="cuda") * 1e-4
        geometry = (tree.scale, tree.depth, tree._on_device("node_index"),
                    tree._on_device("leaf_index"))
        space, sh_space = ops.OctreeGradWorkspace(), ops.OctreeGradSHWorkspace(2)
        k17 = lambda: ops.octree_render_volume_backward(  # noqa: E731
            o, d, *geometry, rows, g, ga, workspace=space)
        k19 = lambda: ops.octree_render_volume_sh_backward(  # noqa: E731
            o, d, *geometry, sh_rows, 2, g, ga, workspace=sh_space)
        k17(), k19()                                    # size the workspaces
        case["backward_k17a_k17b_batch_4096_device_ms"] = device_ms(k17, args.repeats)
        case["backward_k19a_k19b_degree_2_batch_4096_device_ms"] = device_ms(k19, args.repeats)
        write(results)
        case["fit_step_wall_ms"] = {
            "plain_tv_off": step_wall_ms(ffn.fit_octree, tree, train, args.steps),
            "plain_tv_on": step_wall_ms(ffn.fit_octree, tree, train, args.steps,
                                        tv_weight=(1e-3, 1e-3)),
            "sh_degree_2_tv_off": step_wall_ms(ffn.fit_octree_sh, sh_tree, train, args.steps),
            "sh_degree_2_tv_on": step_wall_ms(ffn.fit_octree_sh, sh_tree, train, args.steps,
                                              tv_weight=(1e-3, 1e-3, 1e-3))}
        write(results)
        if depth == args.depths[0]:
            case["psnr_before"] = psnr_pair(tree, val)
            case["total_variation_before"] = tree.total_variation()
            case["held_out"] = []
            for lr in args.learning_rates:
                for weight in [0.0] + list(args.tv_weights):
                    fitted, log = ffn.fit_octree(tree, train, None, 4096, lr, args.fit_steps,
                                                 verbose=False, tv_weight=(weight, weight))
                    losses = [e.loss for e in log]
                    case["held_out"].append({
                        "learning_rate": lr, "tv_weight": [weight, weight],
                        "steps": args.fit_steps, "loss_first_16": float(np.mean(losses[:16])),
                        "loss_last_16": float(np.mean(losses[-16:])),
                        "total_variation_after": fitted.total_variation(),
                        "psnr_after": psnr_pair(fitted, val)})
                    write(results)
        del tree, sh_tree, rows, sh_rows, plan, space, sh_space
        torch.cuda.empty_cache()
    results["complete"] = True
    print(write(results))
    return 0


if __name__ == "__main__":
    sys.exit(main())
