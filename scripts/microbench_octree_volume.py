"""Microbenchmark of the K15 volume render of a baked octree.

The model, the trees and the rays are those of ``scripts/microbench_octree_render.py`` (the voxel
radiance field with an opaque ball, voxelized at depth 8 and 10, the 400x400 rays of the first
training camera); every tree is then baked with the model (``OcTree.bake``).

Per tree:

* wall time (synchronised, best of ``--repeats`` after a warm-up call) and device time (events
  around the launch) of ``render_volume`` with ``min_transmittance`` 0 and 1e-3, and of
  ``first_hit`` and ``spans`` on the same rays;
* wall time of a whole ``render_image(mode="volume")`` frame and, in the same process, of
  ``Raycaster.render_image`` of the model (S = 128 samples per ray);
* the PSNR of the first-hit frame and of the volume frame against the model's frame, over the
  same ``--psnr-cameras`` training cameras (u8 frames, all pixels).

Nothing here asserts a time or a PSNR.

    python scripts/microbench_octree_volume.py [--repeats 5] [--out result.json]
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
from scripts.microbench_octree_render import (SAMPLES, SIDE, coloured_cloud,  # noqa: E402
                                              device_ms, psnr_u8)
from scripts.microbench_octree_walk import SCENE, make_sampler, opaque_ball, wall  # noqa: E402

THRESHOLDS = (0.0, 1e-3)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--repeats", type=int, default=5)
    parser.add_argument("--voxelize-side", type=int, default=800)
    parser.add_argument("--min-leaf-size", type=int, default=1)
    parser.add_argument("--psnr-cameras", type=int, default=4)
    parser.add_argument("--out")
    args = parser.parse_args()
    data = dict(np.load(SCENE))
    n_train = int(data["split_counts"][0])
    model = opaque_ball()
    caster = ffn.Raycaster(model)
    cloud, colors = coloured_cloud(caster, data, list(range(n_train)), args.voxelize_side)
    cameras = list(range(min(args.psnr_cameras, n_train)))
    sampler = make_sampler(data, cameras, SIDE, SAMPLES)
    rays = slice(0, sampler.rays_per_camera)
    model_ms, _ = wall(lambda: caster.render_image(sampler, 0, 16384), args.repeats)
    model_frames = [caster.render_image(sampler, c, 16384) for c in cameras]
    results = {"device": torch.cuda.get_device_name(0), "model": "Voxels(64), opaque ball r=0.45",
               "voxelize": {"cameras": n_train, "side": args.voxelize_side, "samples": SAMPLES,
                            "alpha_threshold": 0.3, "min_leaf_size": args.min_leaf_size,
                            "cloud_points": int(cloud.shape[0])},
               "frame": [SIDE, SIDE], "rays": SIDE * SIDE, "repeats": args.repeats,
               "psnr_cameras": cameras, "model_render_image_wall_ms": model_ms,
               "model_samples_per_ray": SAMPLES, "cases": []}
    for depth in (8, 10):
        tree = ffn.OcTree.build_from_samples(cloud, depth, args.min_leaf_size, colors)
        bake_ms, baked = wall(lambda: tree.bake(model), 1)
        shift = torch.tensor(tree.center, dtype=torch.float32, device="cuda")
        o, d = (sampler.starts[rays] - shift).contiguous(), sampler.directions[rays].contiguous()
        nodes, leaves = baked._on_device("node_index"), baked._on_device("leaf_index")
        leaf_data = baked._colors_on_device()
        geometry = (o, d, baked.scale, baked.depth, nodes, leaves)
        density = baked.leaf_data()[:, 3]
        case = {"tree_depth": baked.depth, "leaves": baked.num_leaves,
                "interior_nodes": len(baked) - baked.num_leaves, "bake_wall_ms": bake_ms,
                "baked_density_min_median_max": [float(density.min()), float(np.median(density)),
                                                 float(density.max())]}
        for threshold in THRESHOLDS:
            key = "render_volume_min_transmittance_%g" % threshold
            ms, out = wall(lambda: baked.render_volume(o, d, min_transmittance=threshold),
                           args.repeats)
            case[key + "_wall_ms"] = ms
            case[key + "_device_ms"] = device_ms(
                lambda: ops.octree_render_volume(*geometry, leaf_data, 0.0, (0.0, 0.0, 0.0),
                                                 threshold), args.repeats)
            case[key + "_mean_alpha"] = float(out.alpha.mean().item())
        case["first_hit_wall_ms"], hit = wall(lambda: baked.first_hit(o, d), args.repeats)
        case["spans_wall_ms"], _ = wall(lambda: baked.spans(o, d, 0.0, 0.0), args.repeats)
        case["first_hit_device_ms"] = device_ms(lambda: ops.octree_first_hit(*geometry, 0.0),
                                                args.repeats)
        case["spans_device_ms"] = device_ms(lambda: ops.octree_spans(*geometry, 0.0, 0.0),
                                            args.repeats)
        case["rays_hitting_a_leaf"] = int((hit.leaves >= 0).sum().item())
        case["volume_render_image_wall_ms"], _ = wall(
            lambda: baked.render_image(sampler, 0, mode="volume"), args.repeats)
        first_frames = [tree.render_image(sampler, c) for c in cameras]
        volume_frames = [baked.render_image(sampler, c, mode="volume") for c in cameras]
        case["psnr_first_hit_frame_vs_model_frame"] = [psnr_u8(a, b) for a, b in
                                                       zip(first_frames, model_frames)]
        case["psnr_volume_frame_vs_model_frame"] = [psnr_u8(a, b) for a, b in
                                                    zip(volume_frames, model_frames)]
        case["mean_psnr_first_hit"] = float(np.mean(case["psnr_first_hit_frame_vs_model_frame"]))
        case["mean_psnr_volume"] = float(np.mean(case["psnr_volume_frame_vs_model_frame"]))
        results["cases"].append(case)
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
