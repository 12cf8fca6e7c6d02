"""Microbenchmark of the K17 octree fit: the backward of the volume render next to its forward,
one ``fit_octree`` step split by kernel, and a few learning rates.

The model and the cameras are those of ``scripts/microbench_octree_density.py`` (the voxel radiance
field with an opaque ball, 400x400 rays of the first training cameras of scene16); the trees are
``OcTree.build_from_model`` at depth 8 and 10.  Per depth:

* device time (events, best of ``--repeats`` after a warm-up call) of ``render_volume`` and of
  K17a + K17b (``ops.octree_render_volume_backward``, its read-back included) on every ray of
  camera 0 and on a 4096-ray batch of shuffled rays, and the number of (ray, taken leaf) entries;
* one ``fit_octree`` step on 4096-ray batches, split by kernel (events), mean of ``--steps``.

The only scene in the repository has 16x16 images, so the targets of the learning-rate trial are the
MODEL's own 400x400 renders (colour and alpha, every ray; black where the sampler has no valid
ray): the depth-8 tree is fitted to ``--fit-cameras`` cameras for ``--fit-steps`` steps per learning
rate, and the PSNR against the model's render of held-out cameras is reported before and after,
over all pixels and where the model's alpha is >= 0.99.  Nothing here asserts a time or a PSNR.

    python scripts/microbench_octree_fit.py [--repeats 5] [--out result.json]
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
from scripts.microbench_octree_render import SAMPLES, SIDE, device_ms  # noqa: E402
from scripts.microbench_octree_walk import SCENE, make_sampler, opaque_ball, render_valid  # noqa: E402


class ModelTargets:
    """What ``fit_octree`` reads of a dataset: the model's own render of every ray."""

    def __init__(self, caster, sampler, alpha_weight=0.1):
        self.sampler, self.alpha_weight = sampler, alpha_weight
        count = len(sampler)
        index = sampler.valid_index(torch.arange(count, device="cuda"))
        color, alpha, _ = render_valid(caster, sampler, index)
        self.colors = torch.zeros((count, 3), dtype=torch.float32, device="cuda")
        self.alphas = torch.zeros((count,), dtype=torch.float32, device="cuda")
        # where the model is transparent its frame shows the colour of its last sample; an octree
        # shows the background, so the target there is colour * alpha
        self.colors[index] = color * alpha[:, None]
        self.alphas[index] = alpha

    def _gt_alphas(self):
        return self.alphas


def psnr_pair(tree, targets):
    sampler = targets.sampler
    shift = torch.tensor(tree.center, dtype=torch.float32, device="cuda")
    out = tree.render_volume((sampler.starts - shift).contiguous(), sampler.directions.contiguous())
    err = ((out.color - targets.colors) ** 2).mean(1).double()
    opaque = targets.alphas >= 0.99
    value = lambda e: float(-10 * np.log10(max(float(e.mean().item()), 1e-12)))  # noqa: E731
    return {"all_pixels": value(err), "where_model_alpha_ge_0.99": value(err[opaque])}


def step_split(tree, targets, steps, lr):
    """``fit_octree``'s step with events between its kernels -> mean device ms per part."""
    field = ffn.OctreeField(tree, tree.center, "cuda")
    data = field.data.detach()
    flat, grads = data.view(-1), torch.empty_like(data)
    m, v = torch.zeros_like(flat), torch.zeros_like(flat)
    sampler = targets.sampler
    shift = torch.tensor(tree.center, dtype=torch.float32, device="cuda")
    tr = field._tree
    nodes, leaves = tr._on_device("node_index"), tr._on_device("leaf_index")
    order = torch.randperm(len(sampler), device="cuda",
                           generator=torch.Generator(device="cuda").manual_seed(1))
    names = ["gather_rays", "forward_k15", "loss_k6", "backward_k17a_k17b", "adam_k7",
             "project_k17c"]
    total = dict.fromkeys(names, 0.0)
    for step in range(steps + 2):
        rays = order[step * 4096:(step + 1) * 4096]
        e = [torch.cuda.Event(enable_timing=True) for _ in range(7)]
        e[0].record()
        starts = (sampler.starts[rays] - shift).contiguous()
        dirs = sampler.directions[rays].contiguous()
        e[1].record()
        color, alpha, _ = ops.octree_render_volume(starts, dirs, tr._scale, tr.depth, nodes,
                                                   leaves, data)
        e[2].record()
        _, d_color, d_alpha = ops.mse_loss(color, alpha, targets.colors, targets.alphas, rays,
                                           1.0 / (3 * 4096), targets.alpha_weight / 4096)
        e[3].record()
        field.backward(starts, dirs, d_color, d_alpha, data=data, out=grads)
        e[4].record()
        ops.clip_adam(flat, grads.view(-1), m, v, step + 1, lr)
        e[5].record()
        ops.octree_project(data)
        e[6].record()
        e[6].synchronize()
        if step >= 2:                                   # two warm-up steps
            for k, name in enumerate(names):
                total[name] += e[k].elapsed_time(e[k + 1]) / steps
    total["whole_step"] = sum(total.values())
    return total


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--repeats", type=int, default=5)
    parser.add_argument("--steps", type=int, default=20)
    parser.add_argument("--depths", type=int, nargs="+", default=[8, 10])
    parser.add_argument("--fit-cameras", type=int, default=8)
    parser.add_argument("--fit-steps", type=int, default=300)
    parser.add_argument("--learning-rates", type=float, nargs="+", default=[1e-3, 1e-2, 1e-1])
    parser.add_argument("--out")
    args = parser.parse_args()
    scene = dict(np.load(SCENE))
    n_train = int(scene["split_counts"][0])
    model = opaque_ball()
    caster = ffn.Raycaster(model)
    fit_cameras = list(range(min(args.fit_cameras, n_train - 2)))
    held_out = [n_train - 2, n_train - 1]
    train = ModelTargets(caster, make_sampler(scene, fit_cameras, SIDE, SAMPLES))
    val = ModelTargets(caster, make_sampler(scene, held_out, SIDE, SAMPLES))
    sampler = train.sampler
    per = sampler.rays_per_camera
    results = {"device": torch.cuda.get_device_name(0), "model": "Voxels(64), opaque ball r=0.45",
               "precision": "f32 (no matrix work on this path; bf16x6 not run)",
               "rocprofv3_kernel_times": "not collected", "frame": [SIDE, SIDE],
               "repeats": args.repeats, "targets": "the model's own render (colour * alpha, alpha)",
               "fit_cameras": fit_cameras, "held_out_cameras": held_out, "cases": []}
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
            g = torch.randn((rays.numel(), 3), device="cuda") * 1e-4
            ga = torch.randn((rays.numel(),), device="cuda") * 1e-4
            space = ops.OctreeGradWorkspace()
            backward = lambda: ops.octree_render_volume_backward(  # noqa: E731
                o, d, *geometry, data, g, ga, workspace=space)
            backward()                                  # sizes the workspace
            forward_ms = device_ms(lambda: ops.octree_render_volume(o, d, *geometry, data),
                                   args.repeats)
            backward_ms = device_ms(backward, args.repeats)
            case["rays"][name] = {"rays": int(rays.numel()), "entries": space.entries,
                                  "render_volume_device_ms": forward_ms,
                                  "backward_k17a_k17b_device_ms": backward_ms,
                                  "backward_over_forward": backward_ms / forward_ms}
        case["fit_step_device_ms"] = step_split(tree, train, args.steps, 1e-2)
        if depth == args.depths[0]:
            case["psnr_before"] = psnr_pair(tree, val)
            case["learning_rates"] = []
            for lr in args.learning_rates:
                fitted, log = ffn.fit_octree(tree, train, None, 4096, lr, args.fit_steps,
                                             verbose=False)
                losses = [e.loss for e in log]
                case["learning_rates"].append({
                    "learning_rate": lr, "steps": args.fit_steps,
                    "loss_first_16": float(np.mean(losses[:16])),
                    "loss_last_16": float(np.mean(losses[-16:])),
                    "psnr_after": psnr_pair(fitted, val)})
        results["cases"].append(case)
        del tree, data
        torch.cuda.empty_cache()
    line = json.dumps(results, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
