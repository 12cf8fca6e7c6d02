"""Microbenchmark of the K13 ray walk and of the empty-space skipping built on it.

The model is a voxel radiance field with an opaque ball in empty space (the one the GPU tests
voxelize).  Trees come from the voxelize flow of ``scripts/voxelize_model.py``: depth renders of
the training cameras of ``tests/golden/scene16.npz`` (at ``--voxelize-side`` pixels), every ray with
``alpha > 0.3`` gives a surface point (K12a-d), ``OcTree.build_from_samples`` at depth 8 and 10.

Per tree and per frame size (400x400, 800x800, the first training camera):

* wall time of ``OcTree.walk`` (max_length 64) and ``OcTree.spans`` on the frame's rays, and, as
  what sample-level skipping would cost without a walker, of ``OcTree.query`` on the same rays x 64
  sample positions;
* wall time of an S = 64 render of the frame through ``RaySampler.clip_to_octree`` and of the
  unclipped S = 64 render, and the PSNR of each against an unclipped S = 256 render of the same
  model (float colours over all pixels of the frame; rays the clipped sampler drops are black).

Wall times are synchronised, best of ``--repeats`` after one warm-up call.  Kernel times come from
a separate run under ``rocprofv3 --kernel-trace --stats`` (a run of its own).

    python scripts/microbench_octree_walk.py [--repeats 3] [--out result.json]
"""

import argparse
import contextlib
import io
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
from fourier_feature_nets_amd.cameras import CameraInfo, Resolution  # noqa: E402

SCENE = os.path.join(ROOT, "tests", "golden", "scene16.npz")
BATCH = 16384


def wall(fn, repeats):
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(repeats):
        start = time.perf_counter()
        result = fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - start)
    return best * 1e3, result


def opaque_ball(side=64):
    model = ffn.Voxels(side, 1.0)
    axis = (np.arange(side) + 0.5) / side * 2 - 1
    x, y, z = np.meshgrid(axis, axis, axis, indexing="ij")
    inside = x * x + y * y + z * z < 0.45 ** 2
    volume = np.random.default_rng(3).normal(size=(1, 4, side, side, side)).astype(np.float32)
    volume[0, 3] = np.where(inside, 12.0, -12.0)
    with torch.no_grad():
        model.voxels.copy_(torch.from_numpy(volume))
        model.bias.zero_()
    return model.to("cuda")


def make_sampler(data, cameras, side, num_samples):
    """The scene's training cameras ``cameras`` at side x side pixels."""
    height, width = data["images"].shape[1:3]
    infos = []
    for c in cameras:
        k = data["intrinsics"][c].astype(np.float32).copy()
        k[0] *= side / width
        k[1] *= side / height
        infos.append(CameraInfo.create("cam%03d" % c, Resolution(side, side), k,
                                       data["extrinsics"][c]))
    with contextlib.redirect_stdout(io.StringIO()):
        return ffn.RaySampler(data["bounds"], infos, num_samples, device="cuda")


def render_valid(caster, sampler, index, want_depth=False):
    """colour (R,3), alpha (R), depth (R) of the valid rays ``index``, in batches."""
    out = []
    with torch.no_grad():
        for start in range(0, index.numel(), BATCH):
            chunk = index[start:start + BATCH].contiguous()
            out.append(caster.render(sampler.sample(chunk, None), want_depth))
    return [torch.cat([o[j] for o in out]) if out[0][j] is not None else None for j in range(3)]


def frame(caster, sampler):
    """(rays, 3) float colours of camera 0, zeros where the sampler has no valid ray."""
    index = sampler._valid_for_camera(0)
    colors = torch.zeros((sampler.rays_per_camera, 3), dtype=torch.float32, device="cuda")
    if index.numel():
        colors[index] = render_valid(caster, sampler, index)[0]
    return colors


def psnr(a, b):
    return float(-10 * torch.log10(((a - b) ** 2).mean()).item())


def surface_cloud(caster, data, cameras, side):
    sampler = make_sampler(data, cameras, side, 128)
    index = sampler.valid_index(torch.arange(len(sampler), device="cuda"))
    color, alpha, depth = render_valid(caster, sampler, index, True)
    positions, _, count = ops.octree_surface_points(
        alpha.contiguous(), depth.contiguous(), sampler.starts[index].contiguous(),
        sampler.directions[index].contiguous(), 0.3)
    return positions[:int(count.item())].contiguous()


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--repeats", type=int, default=3)
    parser.add_argument("--voxelize-side", type=int, default=200)
    parser.add_argument("--min-leaf-size", type=int, default=1)
    parser.add_argument("--out")
    args = parser.parse_args()
    data = dict(np.load(SCENE))
    n_train = int(data["split_counts"][0])
    caster = ffn.Raycaster(opaque_ball())
    cloud = surface_cloud(caster, data, list(range(n_train)), args.voxelize_side)
    results = {"device": torch.cuda.get_device_name(0), "model": "Voxels(64), opaque ball r=0.45",
               "voxelize": {"cameras": n_train, "side": args.voxelize_side, "samples": 128,
                            "alpha_threshold": 0.3, "min_leaf_size": args.min_leaf_size,
                            "cloud_points": int(cloud.shape[0])},
               "max_length": 64, "samples_per_ray_for_query": 64, "cases": []}
    trees = [ffn.OcTree.build_from_samples(cloud, depth, args.min_leaf_size) for depth in (8, 10)]
    for side in (400, 800):
        s64 = make_sampler(data, [0], side, 64)
        s256 = make_sampler(data, [0], side, 256)
        truth = frame(caster, s256)
        plain_ms, plain = wall(lambda: frame(caster, s64), args.repeats)
        plain_psnr = psnr(plain, truth)
        for tree in trees:
            shift = torch.tensor(tree.center, dtype=torch.float32, device="cuda")
            o, d = (s64.starts - shift).contiguous(), s64.directions
            walk_ms, path = wall(lambda: tree.walk(o, d, 64), args.repeats)
            span_ms, (t_in, t_out, hit) = wall(lambda: tree.spans(o, d), args.repeats)
            stops = (path.t_stops < path.t_stops[:, -1:]).sum(1).float()
            near, far = path.t_stops[:, 0], path.t_stops[:, -1]
            t = near[:, None] + (far - near)[:, None] * torch.linspace(0, 1, 64, device="cuda")[None]
            positions = (o[:, None, :] + d[:, None, :] * t[:, :, None]).reshape(-1, 3).contiguous()
            query_ms, answers = wall(lambda: tree.query(positions), args.repeats)
            in_leaf = int((answers >= 0).sum().item())
            del positions, answers, t, path
            clip_ms, clipped = wall(lambda: s64.clip_to_octree(tree, tree.center), args.repeats)
            clipped_ms, image = wall(lambda: frame(caster, clipped), args.repeats)
            valid = clipped.valid != 0
            results["cases"].append({
                "frame": [side, side], "rays": side * side, "tree_depth": tree.depth,
                "leaves": tree.num_leaves, "interior_nodes": len(tree) - tree.num_leaves,
                "walk_wall_ms": walk_ms, "spans_wall_ms": span_ms,
                "query_rays_x_64_wall_ms": query_ms, "query_samples_in_a_leaf": in_leaf,
                "mean_stops_per_ray": float(stops.mean().item()),
                "max_stops_per_ray": int(stops.max().item()),
                "rays_hitting_a_leaf": int(hit.sum().item()),
                "clip_to_octree_wall_ms": clip_ms,
                "valid_rays_unclipped": int((s64.valid != 0).sum().item()),
                "valid_rays_clipped": int(valid.sum().item()),
                "mean_span_clipped": float((clipped.near_far[1] - clipped.near_far[0])[valid].mean().item()),
                "mean_span_unclipped": float((s64.near_far[1] - s64.near_far[0])[valid].mean().item()),
                "render_s64_unclipped_wall_ms": plain_ms, "render_s64_clipped_wall_ms": clipped_ms,
                "psnr_s64_unclipped_vs_s256": plain_psnr,
                "psnr_s64_clipped_vs_s256": psnr(image, truth),
            })
            torch.cuda.empty_cache()
    line = json.dumps(results, indent=1)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
