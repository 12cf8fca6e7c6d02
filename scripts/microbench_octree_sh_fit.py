"""Microbenchmark of the K19 SH octree fit: the backward of the SH volume render next to its
forward, one ``fit_octree_sh`` step split by kernel, and two learning rates.

The tree and the rays are those of ``scripts/microbench_octree_density.py`` and of the K17 and K18
microbenchmarks: the depth-8 density tree of the voxel radiance field with an opaque ball
(``OcTree.build_from_model``), baked with ``bake_sh`` at degrees 1 and 2, and the 400x400 rays of the
first training camera of ``tests/golden/scene16.npz``.  In one process, device time between events,
best of ``--repeats`` after a warm-up call, on every ray of camera 0 and on a 4096-ray batch of
shuffled rays:

* the K18a forward (``ops.octree_render_volume_sh``) and K19a + K19b
  (``ops.octree_render_volume_sh_backward``, its read-back included) per degree, their ratio, and
  the number of (ray, taken leaf) entries;
* for scale, K15 and K17a + K17b on the plain tree, whose ratio the K17 paragraph measured as 2.15;
* one ``fit_octree_sh`` step on 4096-ray batches per degree, split by kernel (events), mean of
  ``--steps``, against the voxel model's own renders.

The learning-rate trial needs a model WITH a view direction: the small NeRF of
``scripts/microbench_octree_sh.py`` (``view_model`` says whether it was trained).  A density tree of
``--view-depth`` built from it is baked with ``bake_sh`` per degree and fitted with
``fit_octree_sh`` for ``--fit-steps`` steps per learning rate to the MODEL's own renders of
``--fit-cameras`` cameras; the training loss (first and last 16 steps) and the PSNR against the
model's render of two held-out cameras, before and after, are recorded.  The default learning rate
of ``fit_octree_sh`` is ``fit_octree``'s; this trial is what says whether it suits logit-space
coefficients.  Nothing here asserts a time or a PSNR, and nothing is tuned after the result.

The result is written after every section, so that a run that is cut short leaves what it had.

    python scripts/microbench_octree_sh_fit.py [--repeats 5] [--out result.json]
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
from fourier_feature_nets_amd import ops  # noqa: E402
from scripts.microbench_octree_fit import ModelTargets, psnr_pair  # noqa: E402
from scripts.microbench_octree_render import SAMPLES, SIDE, device_ms  # noqa: E402
from scripts.microbench_octree_sh import view_model  # noqa: E402
from scripts.microbench_octree_walk import SCENE, make_sampler, opaque_ball  # noqa: E402

K17_BACKWARD_OVER_FORWARD = 2.15        # profiles/r15_octree_fit_microbench.json, depth 8, camera 0


def step_split(tree, targets, steps, lr):
    """``fit_octree_sh``'s step with events between its kernels -> mean device ms per part."""
    field = ffn.OctreeSHField(tree, tree.center, "cuda")
    data = field.data.detach()
    flat, grads = data.view(-1), torch.empty_like(data)
    m, v = torch.zeros_like(flat), torch.zeros_like(flat)
    sampler = targets.sampler
    shift = torch.tensor(tree.center, dtype=torch.float32, device="cuda")
    order = torch.randperm(len(sampler), device="cuda",
                           generator=torch.Generator(device="cuda").manual_seed(1))
    names = ["gather_rays", "forward_k18a", "loss_k6", "backward_k19a_k19b", "adam_k7",
             "project_k19c"]
    total = dict.fromkeys(names, 0.0)
    for step in range(steps + 2):
        rays = order[step * 4096:(step + 1) * 4096]
        e = [torch.cuda.Event(enable_timing=True) for _ in range(7)]
        e[0].record()
        starts = (sampler.starts[rays] - shift).contiguous()
        dirs = sampler.directions[rays].contiguous()
        e[1].record()
        color, alpha, _ = field._render(data, starts, dirs, 0.0, (0.0, 0.0, 0.0), 0.0)
        e[2].record()
        _, d_color, d_alpha = ops.mse_loss(color, alpha, targets.colors, targets.alphas, rays,
                                           1.0 / (3 * 4096), targets.alpha_weight / 4096)
        e[3].record()
        field.backward(starts, dirs, d_color, d_alpha, data=data, out=grads)
        e[4].record()
        ops.clip_adam(flat, grads.view(-1), m, v, step + 1, lr)
        e[5].record()
        ops.octree_project_sh(data, field.sh_degree)
        e[6].record()
        e[6].synchronize()
        if step >= 2:                                   # two warm-up steps
            for k, name in enumerate(names):
                total[name] += e[k].elapsed_time(e[k + 1]) / steps
    total["whole_step"] = sum(total.values())
    return total


def timings(tree, o, d, repeats):
    """Forward and backward of one tree (plain: K15 / K17, SH: K18a / K19) on rays o, d."""
    geometry = (tree.scale, tree.depth, tree._on_device("node_index"), tree._on_device("leaf_index"))
    g = torch.randn((o.shape[0], 3), device="cuda") * 1e-4
    ga = torch.randn((o.shape[0],), device="cuda") * 1e-4
    if tree.sh_degree is None:
        data = tree._colors_on_device()
        space = ops.OctreeGradWorkspace()
        forward = lambda: ops.octree_render_volume(o, d, *geometry, data)  # noqa: E731
        backward = lambda: ops.octree_render_volume_backward(  # noqa: E731
            o, d, *geometry, data, g, ga, workspace=space)
    else:
        rows, degree = tree._sh_rows_on_device(), tree.sh_degree
        space = ops.OctreeGradSHWorkspace(degree)
        forward = lambda: ops.octree_render_volume_sh(o, d, *geometry, rows, degree)  # noqa: E731
        backward = lambda: ops.octree_render_volume_sh_backward(  # noqa: E731
            o, d, *geometry, rows, degree, g, ga, workspace=space)
    backward()                                          # sizes the workspace
    forward_ms, backward_ms = device_ms(forward, repeats), device_ms(backward, repeats)
    return {"rays": int(o.shape[0]), "entries": space.entries, "forward_device_ms": forward_ms,
            "backward_device_ms": backward_ms, "backward_over_forward": backward_ms / forward_ms,
            "workspace_bytes": int(space.buffer.numel()) * 4}


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--repeats", type=int, default=5)
    parser.add_argument("--steps", type=int, default=20)
    parser.add_argument("--depth", type=int, default=8)
    parser.add_argument("--view-depth", type=int, default=7)
    parser.add_argument("--num-views", type=int, default=64)
    parser.add_argument("--train-steps", type=int, default=1000)
    parser.add_argument("--fit-cameras", type=int, default=8)
    parser.add_argument("--fit-steps", type=int, default=300)
    parser.add_argument("--learning-rates", type=float, nargs="+", default=[1e-3, 1e-2])
    parser.add_argument("--out")
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
    fit_cameras = list(range(min(args.fit_cameras, n_train - 2)))
    held_out = [n_train - 2, n_train - 1]
    ball = opaque_ball()
    train = ModelTargets(ffn.Raycaster(ball), make_sampler(scene, fit_cameras, SIDE, SAMPLES))
    sampler = train.sampler
    per = sampler.rays_per_camera
    plain = ffn.OcTree.build_from_model(ball, args.depth, alpha_threshold=0.01)
    trees = {"plain_k15_k17": plain}
    for degree in (1, 2):
        trees["sh_degree_%d" % degree] = plain.bake_sh(ball, degree, args.num_views)
    results = {"device": torch.cuda.get_device_name(0),
               "precision": "f32 (no matrix work on this path; bf16x6 not run)",
               "rocprofv3_kernel_times": "not collected", "frame": [SIDE, SIDE],
               "repeats": args.repeats, "num_views": args.num_views,
               "k17_backward_over_forward_measured_earlier": K17_BACKWARD_OVER_FORWARD,
               "tree": {"model": "Voxels(64), opaque ball r=0.45", "depth": args.depth,
                        "leaves": plain.num_leaves}, "rays": {}, "complete": False}
    shift = torch.tensor(plain.center, dtype=torch.float32, device="cuda")
    shuffled = torch.randperm(len(sampler), device="cuda",
                              generator=torch.Generator(device="cuda").manual_seed(2))[:4096]
    for name, rays in (("camera_0", torch.arange(per, device="cuda")), ("batch_4096", shuffled)):
        o = (sampler.starts[rays] - shift).contiguous()
        d = sampler.directions[rays].contiguous()
        results["rays"][name] = {key: timings(tree, o, d, args.repeats)
                                 for key, tree in trees.items()}
        base = results["rays"][name]["plain_k15_k17"]["backward_over_forward"]
        for degree in (1, 2):
            entry = results["rays"][name]["sh_degree_%d" % degree]
            entry["ratio_minus_k17_ratio_same_run"] = entry["backward_over_forward"] - base
    write(results)
    results["fit_step_device_ms"] = {
        "sh_degree_%d" % degree: step_split(trees["sh_degree_%d" % degree], train, args.steps, 1e-2)
        for degree in (1, 2)}
    write(results)

    # the learning rates, on a model with a view direction
    model, label = view_model(args.train_steps)
    caster = ffn.Raycaster(model)
    fit = {"view_model": label, "depth": args.view_depth, "fit_cameras": fit_cameras,
           "held_out_cameras": held_out, "steps": args.fit_steps, "batch": 4096,
           "targets": "the model's own render (colour * alpha, alpha)",
           "default_learning_rate": ffn.octree_fit.LEARNING_RATE, "degrees": {}}
    results["learning_rates"] = fit
    try:
        view_train = ModelTargets(caster, make_sampler(scene, fit_cameras, SIDE, SAMPLES))
        view_val = ModelTargets(caster, make_sampler(scene, held_out, SIDE, SAMPLES))
        bare = ffn.OcTree.build_from_model(model, args.view_depth)
        fit["leaves"] = bare.num_leaves
        for degree in (1, 2):
            tree = bare.bake_sh(model, degree, args.num_views)
            entry = {"psnr_before": psnr_pair(tree, view_val), "runs": []}
            fit["degrees"]["sh_degree_%d" % degree] = entry
            for lr in args.learning_rates:
                fitted, log = ffn.fit_octree_sh(tree, view_train, None, 4096, lr, args.fit_steps,
                                                verbose=False)
                losses = [e.loss for e in log]
                entry["runs"].append({"learning_rate": lr,
                                      "loss_first_16": float(np.mean(losses[:16])),
                                      "loss_last_16": float(np.mean(losses[-16:])),
                                      "losses_finite": bool(np.isfinite(losses).all()),
                                      "psnr_after": psnr_pair(fitted, view_val)})
                write(results)
    except ValueError as error:             # a model without density has no tree
        fit["error"] = str(error)
    results["complete"] = True
    print(write(results))
    return 0


if __name__ == "__main__":
    sys.exit(main())
