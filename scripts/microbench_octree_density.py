"""Microbenchmark of the K16 density-octree build and of the volume render of its trees.

The model and the cameras are those of ``scripts/microbench_octree_volume.py`` (the voxel radiance
field with an opaque ball, the 400x400 rays of the first training cameras).  Per depth (8 and 10):

* ``OcTree.build_from_model``: wall time of the whole call, and in a loop of its own over the same
  chunks the device time (events) of the model evaluation and of the K16 kernels (centres and
  selection, the count read-back included); wall time of the merge passes; leaf counts with and
  without merging (``--merge-tolerance``);
* wall and device time of ``render_volume`` over one camera's rays, for the density tree, the
  merged density tree and the shell tree (``build_from_samples`` of the depth renders + ``bake``,
  the only route there was before) at the same depth;
* against the model's own render over the same ``--psnr-cameras`` cameras (float colours, the
  sampler's valid rays): PSNR over all pixels, PSNR over the pixels where the model's alpha is
  >= 0.99, mean |alpha difference|, and the share of the summed squared colour error that sits in
  pixels where the model's alpha is < 0.01.  In ``Raycaster.render`` the last sample of a ray has
  a width of 1e10, hence an opacity of 1: its colour always enters ``color`` while ``alpha`` leaves
  it out, so the model's frame is not black off the object and an octree's frame is.
  ``model_color_where_alpha_below_0.01`` records how bright that is.

Nothing here asserts a time or a PSNR.

    python scripts/microbench_octree_density.py [--repeats 3] [--out result.json]
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
from scripts.microbench_octree_render import (SAMPLES, SIDE, coloured_cloud,  # noqa: E402
                                              device_ms)
from scripts.microbench_octree_walk import (SCENE, make_sampler, opaque_ball,  # noqa: E402
                                            render_valid, wall)

BATCH = 1 << 20


def build_split(model, depth, alpha_threshold):
    """The chunk loop of ``build_from_model`` with events around its two halves -> device ms of
    the model evaluation and of K16a + K16b, and the number of kept cells."""
    tau = float(np.float32(-np.log1p(-alpha_threshold)))
    side = 2.0 / 2 ** (depth - 1)
    cells = 8 ** (depth - 1)
    model_ms = k16_ms = 0.0
    kept = 0
    model.eval()
    with torch.no_grad():
        for first in range(0, cells, BATCH):
            count = min(BATCH, cells - first)
            e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            e[0].record()
            points = ops.octree_cell_centers(first, count, (0.0, 0.0, 0.0), 1.0, depth, "cuda")
            e[1].record()
            logits = model(points).reshape(-1, 4).contiguous()
            e[2].record()
            codes, _ = ops.octree_density_select(logits, first, tau, side, depth)
            e[3].record()
            e[3].synchronize()
            k16_ms += e[0].elapsed_time(e[1]) + e[2].elapsed_time(e[3])
            model_ms += e[1].elapsed_time(e[2])
            kept += int(codes.shape[0])
    return model_ms, k16_ms, kept


def psnr(err):
    return float(-10 * np.log10(max(float(err.mean()), 1e-12)))


def compare(tree, starts, dirs, want_c, want_a):
    shift = torch.tensor(tree.center, dtype=torch.float32, device="cuda")
    out = tree.render_volume((starts - shift).contiguous(), dirs)
    err = ((out.color - want_c) ** 2).double().cpu().numpy()
    alpha = want_a.cpu().numpy()
    opaque, clear = alpha >= 0.99, alpha < 0.01
    return {"psnr_all_pixels": psnr(err), "psnr_where_model_alpha_ge_0.99": psnr(err[opaque]),
            "psnr_where_model_alpha_lt_0.01": psnr(err[clear]),
            "mean_abs_alpha_difference": float((out.alpha - want_a).abs().mean().item()),
            "mean_alpha": float(out.alpha.mean().item()),
            "share_of_squared_error_where_model_alpha_lt_0.01":
                float(err[clear].sum() / max(err.sum(), 1e-30)),
            "share_of_squared_error_where_model_alpha_ge_0.99":
                float(err[opaque].sum() / max(err.sum(), 1e-30))}


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--repeats", type=int, default=3)
    parser.add_argument("--voxelize-side", type=int, default=800)
    parser.add_argument("--psnr-cameras", type=int, default=4)
    parser.add_argument("--alpha-threshold", type=float, default=0.01)
    parser.add_argument("--merge-tolerance", type=float, nargs=2, default=[0.01, 0.01])
    parser.add_argument("--depths", type=int, nargs="+", default=[8, 10])
    parser.add_argument("--out")
    args = parser.parse_args()
    data = dict(np.load(SCENE))
    n_train = int(data["split_counts"][0])
    model = opaque_ball()
    caster = ffn.Raycaster(model)
    cloud, colors = coloured_cloud(caster, data, list(range(n_train)), args.voxelize_side)
    cameras = list(range(min(args.psnr_cameras, n_train)))
    sampler = make_sampler(data, cameras, SIDE, SAMPLES)
    index = sampler.valid_index(torch.arange(len(sampler), device="cuda"))
    want_c, want_a, _ = render_valid(caster, sampler, index)
    starts, dirs = sampler.starts[index].contiguous(), sampler.directions[index].contiguous()
    one = index[index < sampler.rays_per_camera]
    o1, d1 = sampler.starts[one].contiguous(), sampler.directions[one].contiguous()
    clear = want_a < 0.01
    results = {"device": torch.cuda.get_device_name(0), "model": "Voxels(64), opaque ball r=0.45",
               "precision": "f32 (bf16x6 unmeasured)", "rocprofv3_kernel_times": "unmeasured",
               "frame": [SIDE, SIDE], "cameras": cameras, "valid_rays": int(index.numel()),
               "rays_of_camera_0": int(one.numel()), "model_samples_per_ray": SAMPLES,
               "alpha_threshold": args.alpha_threshold, "merge_tolerance": args.merge_tolerance,
               "batch_size": BATCH, "repeats": args.repeats,
               "pixels_where_model_alpha_ge_0.99": int((want_a >= 0.99).sum().item()),
               "pixels_where_model_alpha_lt_0.01": int(clear.sum().item()),
               "model_color_where_alpha_below_0.01": {
                   "mean": float(want_c[clear].mean().item()),
                   "max": float(want_c[clear].max().item()),
                   "mean_square": float((want_c[clear] ** 2).mean().item())},
               "shell_voxelize": {"cameras": n_train, "side": args.voxelize_side,
                                  "alpha_threshold": 0.3, "min_leaf_size": 1,
                                  "cloud_points": int(cloud.shape[0])},
               "cases": []}
    for depth in args.depths:
        build = lambda tol=None: ffn.OcTree.build_from_model(  # noqa: E731
            model, depth, alpha_threshold=args.alpha_threshold, merge_tolerance=tol)
        build_ms, dense = wall(build, 1)
        model_ms, k16_ms, kept = build_split(model, depth, args.alpha_threshold)
        start = time.perf_counter()
        merged = build(tuple(args.merge_tolerance))
        torch.cuda.synchronize()
        merged_ms = (time.perf_counter() - start) * 1e3
        shell = ffn.OcTree.build_from_samples(cloud, depth, 1, colors).bake(model)
        case = {"depth": depth, "finest_cells": 8 ** (depth - 1),
                "build_from_model_wall_ms": build_ms,
                "build_from_model_with_merging_wall_ms": merged_ms,
                "model_evaluation_device_ms": model_ms, "k16a_k16b_device_ms": k16_ms,
                "leaves": dense.num_leaves, "kept_cells_in_split_loop": kept,
                "leaves_with_merging": merged.num_leaves,
                "interior_nodes": len(dense) - dense.num_leaves,
                "interior_nodes_with_merging": len(merged) - merged.num_leaves,
                "shell_leaves": shell.num_leaves, "trees": {}}
        for name, tree in (("density", dense), ("density_merged", merged), ("shell", shell)):
            shift = torch.tensor(tree.center, dtype=torch.float32, device="cuda")
            o = (o1 - shift).contiguous()
            entry = compare(tree, starts, dirs, want_c, want_a)
            entry["render_volume_wall_ms"], _ = wall(lambda: tree.render_volume(o, d1),
                                                     args.repeats)
            geometry = (o, d1, tree.scale, tree.depth, tree._on_device("node_index"),
                        tree._on_device("leaf_index"))
            leaf_data = tree._colors_on_device()
            entry["render_volume_device_ms"] = device_ms(
                lambda: ops.octree_render_volume(*geometry, leaf_data), args.repeats)
            case["trees"][name] = entry
        results["cases"].append(case)
        del dense, merged, shell
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
