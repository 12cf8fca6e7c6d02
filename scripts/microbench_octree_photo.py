"""Microbenchmark of K28, carving by photo-consistency (``OcTree.visible_moments`` /
``carve_photo`` / ``build_from_silhouettes(photo_threshold=...)``), on the dataset of
``scripts/microbench_octree_carve.py`` (the procedural torus, 120 cameras of 400 x 400).
Recorded, nothing asserted, nothing tuned afterwards:

* kernel cost: K28a next to K24 on the same inputs in the same process, the C entry points alone
  (events, best of ``--repeats`` after a warm-up), at depth 8 and 10 with the first 8 and all 120
  cameras, trees carved from all cameras with the defaults; both times, their ratio, and the share
  of the (leaf, camera) pairs that end visible (the pairs that send atomics);
* the experiment, K23's protocol: depth 8, 116 training cameras, 4 held out, every pixel of theirs
  against the ground-truth frame.  Four carves -- the point carve and the box carve, each from the
  116 training cameras and from the first 8 of them -- and per carve the arm without photo carving
  (``color_from_images``, which is ``color="visible"``) and ``photo_threshold`` 0.05, 0.1 and 0.2
  (``carve_photo(recolor=True)`` on the unmerged hull with ``min_transmittance = 0.3``, which is
  ``build_from_silhouettes(photo_threshold=..., color="visible")``; judged by the cameras that
  carved).  Per arm: the sweep report, leaves before and after, the wall time of the sweeps, the
  held-out PSNR as built and after 300 ``fit_octree`` steps at the defaults on the 116 cameras;
* completeness: the protocol of ``scripts/skip_from_silhouettes_demo.py`` at resolution 128, grid
  ``dilate`` 0 and 1: how many bits of the analytic grid the grid of each photo-carved tree lacks,
  next to the uncarved tree's figure, for both footprints.

The result file is rewritten after every arm, so a run that is cut short leaves what it measured.

    python scripts/microbench_octree_photo.py [--repeats 5] [--out result.json]
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
from fourier_feature_nets_amd import ops  # noqa: E402
from scripts.microbench_octree_carve import (FIT_STEPS, HELD_OUT, psnr_all_pixels, quiet,  # noqa: E402
                                             torus_dataset)
from scripts.microbench_octree_carve_box import bit_count  # noqa: E402
from scripts.microbench_octree_render import device_ms  # noqa: E402
from scripts.microbench_octree_visible import ALPHA_U8, TAU, k24_inputs  # noqa: E402

DEFAULT_OUT = os.path.join(ROOT, "profiles", "r26_octree_photo_microbench.json")
THRESHOLDS = (0.05, 0.1, 0.2)


def kernel_case(tree, images_u8, cameras, center, repeats):
    """K24 and K28a, the entry points alone, on the same inputs."""
    args = k24_inputs(tree, images_u8, cameras, center)
    leaves, count = tree.num_leaves, len(cameras)
    dev = images_u8.device
    blocks = torch.cat([args[9].reshape(count, 12), args[10],
                        torch.zeros((count, 1), device=dev)], 1).contiguous()
    height, width = images_u8.shape[1:3]
    case = {"depth": tree.depth, "cameras": count, "leaves": leaves, "pairs": leaves * count}
    for entry, fields, key in (("ffn_octree_visible_votes", 4, "k24"),
                               ("ffn_octree_visible_moments", 8, "k28a")):
        out = torch.zeros((leaves, fields), dtype=torch.uint32, device=dev)

        def launch():
            ops._call(entry, ops._dev(args[0]), ops.c_i64(leaves), ops.c_f(tree.scale),
                      ops.c_i(tree.depth), ops._dev(args[3], torch.int64),
                      ops.c_i64(args[3].numel()), ops._dev(args[4], torch.int64),
                      ops._dev(args[5]), ops.c_i(4), ops.c_i(3), ops._dev(images_u8, torch.uint8),
                      ops._dev(blocks), ops.c_i(count), ops.c_i(height), ops.c_i(width),
                      ops.c_i(ALPHA_U8), ops.c_f(TAU), ops._dev(out, torch.uint32))
        case[key + "_device_ms"] = device_ms(launch, repeats)
    case["k28a_over_k24"] = case["k28a_device_ms"] / case["k24_device_ms"]
    moments = ops.octree_visible_moments(*args).cpu().numpy().astype(np.int64)
    votes = ops.octree_visible_votes(*args).cpu().numpy().astype(np.int64)
    case["first_four_fields_equal_k24"] = bool(np.array_equal(moments[:, :4], votes))
    case["share_of_pairs_visible"] = float(votes[:, 3].sum()) / (leaves * count)
    case["k28a_pairs_per_s"] = leaves * count / (case["k28a_device_ms"] * 1e-3)
    return case


def report_rows(report):
    return {"sweeps": [list(s) for s in report], "converged": bool(report.converged)}


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--repeats", type=int, default=5)
    parser.add_argument("--depths", type=int, nargs="*", default=[8, 10])
    parser.add_argument("--camera-counts", type=int, nargs="+", default=[8, 120])
    parser.add_argument("--size", type=int, default=400)
    parser.add_argument("--truth-depth", type=int, default=9)
    parser.add_argument("--fit-depth", type=int, default=8)
    parser.add_argument("--few", type=int, default=8, help="cameras of the few-view carves")
    parser.add_argument("--skip-experiment", action="store_true")
    parser.add_argument("--skip-completeness", action="store_true")
    parser.add_argument("--out", default=DEFAULT_OUT)
    args = parser.parse_args()
    num_cameras = max(args.camera_counts)
    truth, images, cameras, bounds = torus_dataset(num_cameras, args.size, args.truth_depth)
    center, scale = truth.center, truth.scale
    results = {"device": torch.cuda.get_device_name(0),
               "dataset": "procedural_torus() at depth %d (%d leaves), %d cameras of %d x %d, "
                          "first-hit frames" % (args.truth_depth, truth.num_leaves, num_cameras,
                                                args.size, args.size),
               "cube": {"center": list(center), "scale": scale},
               "settings": "carves with the defaults (alpha_threshold 0.5, dilate 1, max_misses 0, "
                           "min_views 2, cell_opacity 0.5, no merging); alpha_u8 %d, "
                           "min_transmittance %g, photo min_views 2, max_sweeps 16"
                           % (ALPHA_U8, TAU),
               "repeats": args.repeats,
               "not_measured": "rocprofv3 kernel times; --precision bf16x6 (no matrix work on this "
                               "path); other scenes; real photographs",
               "kernel_cost": []}

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(results, indent=1) + "\n")

    dev = torch.device("cuda")
    whole = argparse.Namespace(images=images, cameras=cameras, color_space="RGB")
    for depth in args.depths:
        tree = ffn.OcTree.build_from_silhouettes(whole, depth, center, scale)
        for count in args.camera_counts:
            images_u8 = torch.from_numpy(np.ascontiguousarray(images[:count])).to(dev)
            case = kernel_case(tree, images_u8, cameras[:count], center, args.repeats)
            results["kernel_cost"].append(case)
            print(json.dumps(case), flush=True)
            del images_u8
            torch.cuda.empty_cache()
        del tree
        torch.cuda.empty_cache()
        write()
    if not args.skip_completeness:
        completeness(results)
        write()
    if not args.skip_experiment:
        experiment(results, write, images, cameras, bounds, center, scale, num_cameras, args)
    write()
    return 0


def experiment(results, write, images, cameras, bounds, center, scale, num_cameras, args):
    train_n = num_cameras - HELD_OUT
    train = quiet(ffn.ImageDataset, "train", images[:train_n], bounds, cameras[:train_n], 8,
                  device="cuda")
    held = quiet(ffn.ImageDataset, "val", images[train_n:], bounds, cameras[train_n:], 8,
                 device="cuda")
    few = argparse.Namespace(images=images[:args.few], cameras=cameras[:args.few],
                             color_space="RGB")

    def psnr(tree):
        return psnr_all_pixels(lambda starts, dirs: tree.render_volume(starts, dirs).color, held,
                               center)

    out = {"depth": args.fit_depth, "train_cameras": train_n, "held_out_cameras": HELD_OUT,
           "fit_steps": FIT_STEPS, "few_view_cameras": args.few,
           "note": "every arm is carved, photo-carved and recoloured from the cameras of its "
                   "carve, and fitted on all training cameras", "arms": []}
    results["experiment"] = out
    for footprint, carvers, name in (("point", train, "point_116"), ("box", train, "box_116"),
                                     ("point", few, "point_%d" % args.few),
                                     ("box", few, "box_%d" % args.few)):
        hull = ffn.OcTree.build_from_silhouettes(carvers, args.fit_depth, center, scale,
                                                 footprint=footprint)
        hull.carve_photo(carvers, center, 1.0, max_sweeps=1)          # warm-up
        for threshold in (None,) + THRESHOLDS:
            torch.cuda.synchronize()
            start = time.perf_counter()
            if threshold is None:
                tree, report = hull.color_from_images(carvers, center)[0], None
            else:
                tree, report = hull.carve_photo(carvers, center, threshold, recolor=True)
            torch.cuda.synchronize()
            wall = 1e3 * (time.perf_counter() - start)
            arm = {"carve": name, "photo_threshold": threshold, "leaves_before": hull.num_leaves,
                   "leaves_after": tree.num_leaves, "wall_ms": wall,
                   "psnr_as_built": psnr(tree)}
            if report is not None:
                arm.update(report_rows(report))
            fitted, log = ffn.fit_octree(tree, train, None, num_steps=FIT_STEPS, verbose=False)
            arm["psnr_after_fit_octree"] = psnr(fitted)
            arm["fit_loss_first_last"] = [log[0].loss, log[-1].loss]
            out["arms"].append(arm)
            print(json.dumps(arm), flush=True)
            del fitted, tree
            torch.cuda.empty_cache()
            write()
    del train, held
    torch.cuda.empty_cache()


def completeness(results):
    import skip_training_demo as protocol
    scene = protocol.make_scene(protocol.parse_args([]), torch.device("cuda:0"))
    analytic = scene.analytic.bits
    total = bit_count(analytic)
    out = {"analytic_bits": total, "resolution": 128, "depth": 8, "grids": []}
    results["completeness"] = out
    for footprint in ("point", "box"):
        for threshold in (None,) + THRESHOLDS:
            for dilate in (0, 1):
                report = ffn.PhotoReport()
                grid = ffn.OccupancyGrid.from_silhouettes(
                    scene.train, resolution=128, depth=8, dilate=dilate, footprint=footprint,
                    photo_threshold=threshold, photo_report=report)
                lacking = bit_count(analytic & ~grid.bits)
                row = {"footprint": footprint, "photo_threshold": threshold, "grid_dilate": dilate,
                       "bits": bit_count(grid.bits), "bits_of_the_analytic_grid_it_lacks": lacking,
                       "share_of_the_analytic_grid_it_lacks": lacking / max(total, 1)}
                if threshold is not None:
                    row.update(report_rows(report))
                out["grids"].append(row)
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    sys.exit(main())
