"""Microbenchmark of the K14 first-hit render of a voxelized model.

The model is the voxel radiance field with an opaque ball in empty space that
``scripts/microbench_octree_walk.py`` uses, and the trees come from the same voxelize flow (depth
renders of the training cameras of ``tests/golden/scene16.npz`` at ``--voxelize-side`` pixels, every
ray with ``alpha > 0.3`` gives a coloured surface point, ``OcTree.build_from_samples`` at depth 8
and 10).

Per tree, on the 400x400 rays of the first training camera:

* wall time (synchronised, best of ``--repeats`` after a warm-up call) and device time (events
  around the launch, outputs allocated outside) of ``first_hit``, ``render`` and ``spans``;
* wall time of ``OcTree.render_image`` and, in the same process, of ``Raycaster.render_image`` of
  the model the tree came from (S = 128 samples per ray), and the PSNR of the octree frame against
  that model frame (u8 frames, all pixels).

    python scripts/microbench_octree_render.py [--repeats 5] [--out result.json]
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
from scripts.microbench_octree_walk import (SCENE, make_sampler, opaque_ball,  # noqa: E402
                                            render_valid, wall)

SIDE = 400
SAMPLES = 128


def device_ms(fn, repeats):
    """Best time between two events around ``fn`` (a single launch), after one warm-up call."""
    fn()
    best = float("inf")
    for _ in range(repeats):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        end.record()
        end.synchronize()
        best = min(best, start.elapsed_time(end))
    return best


def coloured_cloud(caster, data, cameras, side):
    sampler = make_sampler(data, cameras, side, SAMPLES)
    index = sampler.valid_index(torch.arange(len(sampler), device="cuda"))
    color, alpha, depth = render_valid(caster, sampler, index, True)
    positions, kept, count = ops.octree_surface_points(
        alpha.contiguous(), depth.contiguous(), sampler.starts[index].contiguous(),
        sampler.directions[index].contiguous(), 0.3, color.contiguous())
    count = int(count.item())
    return positions[:count].contiguous(), kept[:count].contiguous()


def psnr_u8(a, b):
    err = ((a.astype(np.float64) - b.astype(np.float64)) / 255.0) ** 2
    return float(-10 * np.log10(max(err.mean(), 1e-12)))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--repeats", type=int, default=5)
    # 800 pixels: a pixel's footprint on the ball (~0.004) is below the side of a depth-8 cell
    # (0.007), so that tree has no holes; at 200 pixels (the walk microbenchmark) it has
    parser.add_argument("--voxelize-side", type=int, default=800)
    parser.add_argument("--min-leaf-size", type=int, default=1)
    parser.add_argument("--out")
    args = parser.parse_args()
    data = dict(np.load(SCENE))
    n_train = int(data["split_counts"][0])
    caster = ffn.Raycaster(opaque_ball())
    cloud, colors = coloured_cloud(caster, data, list(range(n_train)), args.voxelize_side)
    sampler = make_sampler(data, [0], SIDE, SAMPLES)
    model_ms, model_frame = wall(lambda: caster.render_image(sampler, 0, 16384), args.repeats)
    results = {"device": torch.cuda.get_device_name(0), "model": "Voxels(64), opaque ball r=0.45",
               "voxelize": {"cameras": n_train, "side": args.voxelize_side, "samples": SAMPLES,
                            "alpha_threshold": 0.3, "min_leaf_size": args.min_leaf_size,
                            "cloud_points": int(cloud.shape[0])},
               "frame": [SIDE, SIDE], "rays": SIDE * SIDE, "repeats": args.repeats,
               "model_render_image_wall_ms": model_ms, "model_samples_per_ray": SAMPLES,
               "cases": []}
    for depth in (8, 10):
        tree = ffn.OcTree.build_from_samples(cloud, depth, args.min_leaf_size, colors)
        shift = torch.tensor(tree.center, dtype=torch.float32, device="cuda")
        o, d = (sampler.starts - shift).contiguous(), sampler.directions.contiguous()
        nodes, leaves = tree._on_device("node_index"), tree._on_device("leaf_index")
        leaf_data = tree._colors_on_device()
        geometry = (o, d, tree.scale, tree.depth, nodes, leaves)
        hit_wall, hit = wall(lambda: tree.first_hit(o, d), args.repeats)
        render_wall, _ = wall(lambda: tree.render(o, d), args.repeats)
        faces_wall, _ = wall(lambda: tree.render(o, d, shading="faces"), args.repeats)
        spans_wall, (_, _, span_hit) = wall(lambda: tree.spans(o, d, 0.0, 0.0), args.repeats)
        image_wall, frame = wall(lambda: tree.render_image(sampler, 0), args.repeats)
        assert torch.equal(hit.leaves >= 0, span_hit)
        # how far each kernel walks: regions up to the first leaf / over the whole chord
        length = 3 * 2 ** (tree.depth - 1) + 2 if tree.depth <= 8 else 256
        path = tree.walk(o, d, length)
        stops = (path.t_stops < path.t_stops[:, -1:]).sum(1)
        first = torch.where(hit.leaves >= 0, ((path.leaves >= 0).float().argmax(1) + 1), stops)
        results["cases"].append({
            "tree_depth": tree.depth, "leaves": tree.num_leaves,
            "interior_nodes": len(tree) - tree.num_leaves,
            "rays_hitting_a_leaf": int((hit.leaves >= 0).sum().item()),
            "first_hit_wall_ms": hit_wall, "render_flat_wall_ms": render_wall,
            "render_faces_wall_ms": faces_wall, "spans_wall_ms": spans_wall,
            "first_hit_device_ms": device_ms(lambda: ops.octree_first_hit(*geometry, 0.0),
                                             args.repeats),
            "render_flat_device_ms": device_ms(
                lambda: ops.octree_render(*geometry, leaf_data, 0.0), args.repeats),
            "spans_device_ms": device_ms(lambda: ops.octree_spans(*geometry, 0.0, 0.0),
                                         args.repeats),
            "mean_regions_to_first_hit": float(first.float().mean().item()),
            "mean_regions_on_the_chord": float(stops.float().mean().item()),
            "regions_counted_up_to": length - 1,
            "octree_render_image_wall_ms": image_wall,
            "psnr_octree_frame_vs_model_frame": psnr_u8(frame, model_frame),
        })
        del path
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
