"""Microbenchmark of K23, space carving (``OcTree.build_from_silhouettes``), and the experiment it
exists for: an octree from a dataset's images alone, then fitted.

The dataset is the one ``scripts/make_mesh_npz.py`` writes for the procedural torus, made in
memory: the torus as a depth-9 colour tree (K22), rendered by the first-hit walk from the
benchmark's synthetic rig (120 cameras, 400 x 400), alpha 255 where a ray hit, the cameras in that
script's seeded order.  The carved cube is the ground-truth tree's (``center``, ``scale``).
Recorded, nothing asserted, nothing tuned afterwards:

* per depth (8 and 10) and camera count (the first 8, all 120): the device time of the K23 entry
  point (projection kernel, scan and scatter; events, best of ``--repeats`` after a warm-up, per
  chunk of 2^20 cells and summed), the wall time of the whole build, the leaves kept out of how
  many cells, and the mean number of cameras a cell's loop looked at;
* the experiment, at depth 8: carve from all but the last 4 cameras, hold those 4 out, every pixel
  of theirs against the ground-truth frame (colour, black background): the PSNR of the carved tree
  as built, after ``fit_octree`` for 300 steps at the default learning rate, after
  ``fit_octree_adaptive(rounds=1)`` with 300 steps per fit, and next to them the PSNR of the
  ground-truth K22 tree built at the same depth (first-hit render: its leaves are opaque cells).

    python scripts/microbench_octree_carve.py [--repeats 5] [--out result.json]
"""

import argparse
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fourier_feature_nets_amd as ffn  # noqa: E402
from fourier_feature_nets_amd import ops  # noqa: E402
from scripts.microbench_octree_refine import wall_ms  # noqa: E402
from scripts.microbench_octree_render import device_ms  # noqa: E402

DEFAULT_OUT = os.path.join(ROOT, "profiles", "r21_octree_carve_microbench.json")
CHUNK = 1 << 20
HELD_OUT = 4
FIT_STEPS = 300


def quiet(fn, *args, **kwargs):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*args, **kwargs)


def torus_dataset(num_cameras, size, truth_depth):
    """What make_mesh_npz.py writes, in memory -> (truth tree, images, cameras, bounds)."""
    from bench import synthetic_rig
    truth = ffn.OcTree.build_from_triangles(*ffn.procedural_torus(), truth_depth, 4)
    intr, poses = synthetic_rig(num_cameras, size)
    cameras = [ffn.CameraInfo.create("c%03d" % i, ffn.Resolution(size, size), intr, p)
               for i, p in enumerate(poses)]
    bounds = np.diag([2, 2, 2, 1]).astype(np.float32)
    sampler = quiet(ffn.RaySampler, bounds, cameras, 8)
    images = np.zeros((num_cameras, size, size, 4), np.uint8)
    for index in range(num_cameras):
        color, alpha, _ = truth.render_image(sampler, index, shading="flat", include_depth=True)
        images[index, ..., :3] = color
        images[index, ..., 3] = np.where(alpha > 0, 255, 0)
    order = torch.randperm(num_cameras, generator=torch.Generator().manual_seed(0)).numpy()
    return truth, images[order], [cameras[i] for i in order], bounds


def kernel_case(images_u8, mask_u8, proj, center, scale, depth, repeats):
    """Device time of the K23 entry point chunk by chunk, and what the cells' loops looked at."""
    cells = 8 ** (depth - 1)
    side = float(np.float32(2.0 * scale) / np.float32(2.0 ** (depth - 1)))
    sigma0 = float(np.float32(-np.log1p(-0.5) / side))
    dev = images_u8.device
    cameras, height, width = mask_u8.shape
    rows = torch.empty((CHUNK, 4), dtype=torch.float32, device=dev)
    codes = torch.empty((CHUNK,), dtype=torch.int32, device=dev)
    data = torch.empty((CHUNK, 4), dtype=torch.float32, device=dev)
    total = torch.zeros((), dtype=torch.int32, device=dev)
    visited = torch.empty((CHUNK,), dtype=torch.int32, device=dev)
    flags, offsets, tiles = ops._scan_scratch(CHUNK, dev)
    times, looked, kept = [], 0, 0
    for first in range(0, cells, CHUNK):
        count = min(CHUNK, cells - first)

        def launch():
            ops._call("ffn_octree_carve_select", ops._dev(images_u8, torch.uint8),
                      ops._dev(mask_u8, torch.uint8), ops._dev(proj), ops.c_i(cameras),
                      ops.c_i(height), ops.c_i(width), ops.c_i64(first), ops.c_i64(count),
                      ops.c_f(center[0]), ops.c_f(center[1]), ops.c_f(center[2]), ops.c_f(scale),
                      ops.c_i(depth), ops.c_i(128), ops.c_i(0), ops.c_i(2), ops.c_f(sigma0),
                      ops._dev(flags, torch.uint8), ops._dev(offsets, torch.int32),
                      ops._dev(tiles, torch.int32), ops._dev(rows), ops._dev(visited, torch.int32),
                      ops._dev(codes, torch.int32), ops._dev(data), ops._dev(total, torch.int32))
        times.append(device_ms(launch, repeats))
        looked += int(visited[:count].sum(dtype=torch.int64).item())
        kept += int(total.item())
    return {"chunks": len(times), "k23_device_ms_total": float(np.sum(times)),
            "k23_device_ms_per_chunk_min_median_max": [float(np.min(times)),
                                                       float(np.median(times)),
                                                       float(np.max(times))],
            "cells": cells, "cells_kept_by_the_kernel": kept,
            "mean_cameras_visited_per_cell": looked / cells}


def psnr_all_pixels(render, dataset, center):
    """Colour PSNR over every pixel of the dataset's cameras, black background."""
    sampler = dataset.sampler
    shift = torch.tensor(center, dtype=torch.float32, device=sampler.starts.device)
    per = sampler.rays_per_camera
    error = 0.0
    for camera in range(sampler.num_cameras):
        rays = slice(camera * per, (camera + 1) * per)
        color = render((sampler.starts[rays] - shift).contiguous(),
                       sampler.directions[rays].contiguous())
        error += float(((color - dataset.colors[rays]) ** 2).sum(dtype=torch.float64).item())
    return float(-10 * np.log10(max(error / (3 * per * sampler.num_cameras), 1e-12)))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--repeats", type=int, default=5)
    parser.add_argument("--depths", type=int, nargs="+", default=[8, 10])
    parser.add_argument("--camera-counts", type=int, nargs="+", default=[8, 120])
    parser.add_argument("--size", type=int, default=400)
    parser.add_argument("--truth-depth", type=int, default=9)
    parser.add_argument("--fit-depth", type=int, default=8)
    parser.add_argument("--out", default=DEFAULT_OUT)
    args = parser.parse_args()
    num_cameras = max(args.camera_counts)
    truth, images, cameras, bounds = torus_dataset(num_cameras, args.size, args.truth_depth)
    center, scale = truth.center, truth.scale
    results = {"device": torch.cuda.get_device_name(0),
               "dataset": "procedural_torus() at depth %d (%d leaves), %d cameras of %d x %d, "
                          "first-hit frames, hit share %.3f"
                          % (args.truth_depth, truth.num_leaves, num_cameras, args.size, args.size,
                             float((images[..., 3] > 0).mean())),
               "cube": {"center": list(center), "scale": scale},
               "defaults": "alpha_threshold 0.5, dilate 1, max_misses 0, min_views 2, "
                           "cell_opacity 0.5, no merging; chunks of 2^20 cells",
               "repeats": args.repeats, "rocprofv3_kernel_times": "not collected", "cases": []}
    dev = torch.device("cuda")
    for count in args.camera_counts:
        scene = argparse.Namespace(images=images[:count], cameras=cameras[:count],
                                   color_space="RGB")
        images_u8 = torch.from_numpy(np.ascontiguousarray(scene.images)).to(dev)
        mask = (images_u8[..., 3] >= 128).to(torch.float32)
        mask_u8 = torch.nn.functional.max_pool2d(mask[:, None], 3, stride=1,
                                                 padding=1)[:, 0].to(torch.uint8).contiguous()
        proj = torch.from_numpy(ffn.projection_matrices(scene.cameras)).to(dev)
        for depth in args.depths:
            case = {"depth": depth, "cameras": count}
            case.update(kernel_case(images_u8, mask_u8, proj, center, scale, depth, args.repeats))

            def build():
                return ffn.OcTree.build_from_silhouettes(scene, depth, center, scale)
            tree = build()
            case["leaves"] = tree.num_leaves
            del tree
            case["build_from_silhouettes_wall_ms"] = wall_ms(build, args.repeats)
            results["cases"].append(case)
            print(json.dumps(case), flush=True)
            torch.cuda.empty_cache()
        del images_u8, mask_u8, proj
    # ---- the experiment
    train_n = num_cameras - HELD_OUT
    train = quiet(ffn.ImageDataset, "train", images[:train_n], bounds, cameras[:train_n], 8,
                  device="cuda")
    held = quiet(ffn.ImageDataset, "val", images[train_n:], bounds, cameras[train_n:], 8,
                 device="cuda")
    depth = args.fit_depth
    carved = ffn.OcTree.build_from_silhouettes(train, depth, center, scale)

    def volume(tree):
        return lambda starts, dirs: tree.render_volume(starts, dirs).color

    experiment = {"depth": depth, "train_cameras": train_n, "held_out_cameras": HELD_OUT,
                  "fit_steps": FIT_STEPS, "carved_leaves": carved.num_leaves,
                  "psnr_carved_as_built": psnr_all_pixels(volume(carved), held, center)}
    fitted, log = ffn.fit_octree(carved, train, None, num_steps=FIT_STEPS, verbose=False)
    experiment["psnr_after_fit_octree"] = psnr_all_pixels(volume(fitted), held, center)
    experiment["fit_loss_first_last"] = [log[0].loss, log[-1].loss]
    adapted, _, reports = ffn.fit_octree_adaptive(carved, train, None, rounds=1,
                                                  num_steps=FIT_STEPS, verbose=False)
    experiment["psnr_after_fit_octree_adaptive_1_round"] = psnr_all_pixels(volume(adapted), held,
                                                                          center)
    experiment["adaptive_leaves"] = adapted.num_leaves
    experiment["adaptive_report"] = ffn.octree_fit.format_refine_report(reports[0])
    same_depth = ffn.OcTree.build_from_triangles(*ffn.procedural_torus(), depth, 4)
    experiment["ground_truth_tree_leaves"] = same_depth.num_leaves
    experiment["psnr_ground_truth_k22_tree_first_hit"] = psnr_all_pixels(
        lambda starts, dirs: same_depth.render(starts, dirs).color, held, same_depth.center)
    results["experiment"] = experiment
    line = json.dumps(results, indent=1)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
