"""Microbenchmark of K27, the conservative coarse-to-fine carve
(``OcTree.build_from_silhouettes(footprint="box")``), next to K23's point carve in the same
process, on the dataset of ``scripts/microbench_octree_carve.py`` (the procedural torus, 120 cameras
of 400 x 400).  Recorded, nothing asserted, nothing tuned afterwards:

* per depth (8 and 10, and 11 for ``"box"`` alone if it fits in memory) and camera count (the
  first 8, all 120), for both footprints: the device time of the entry points (events round every
  call of the C entry point during one build, summed; best of ``--repeats`` builds), the wall
  time of the build (best of ``--repeats``), the leaves, and for ``"box"`` the candidates and
  survivors of every level, how many leaves it keeps that ``"point"`` does not, and the share of
  its leaves that start grey;
* held-out PSNR under K23's protocol: depth 8, all but the last 4 cameras, those 4 held out, as
  built and after 300 ``fit_octree`` steps, for both footprints;
* occupancy bits: how many bits of the analytic grid of ``scripts/skip_training_demo.py`` a
  ``OccupancyGrid.from_silhouettes`` grid lacks at ``dilate = 0`` (and at the earlier protocol's
  ``dilate = 1``), for both footprints.

    python scripts/microbench_octree_carve_box.py [--repeats 5] [--out result.json]
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

DEFAULT_OUT = os.path.join(ROOT, "profiles", "r25_octree_carve_box_microbench.json")
ENTRY_POINTS = ("ffn_octree_carve_select", "ffn_octree_carve_box_level")


class EntryPointTimer:
    """Events round every call of the carve entry points while it is active."""

    def __enter__(self):
        self.pairs, self.inner = [], ops._call

        def timed(name, *args):
            if name not in ENTRY_POINTS:
                return self.inner(name, *args)
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            result = self.inner(name, *args)
            end.record()
            self.pairs.append((start, end))
            return result
        ops._call = timed
        return self

    def __exit__(self, *exc):
        ops._call = self.inner
        torch.cuda.synchronize()
        self.calls = len(self.pairs)
        self.device_ms = float(sum(a.elapsed_time(b) for a, b in self.pairs))


def build_case(scene, depth, center, scale, footprint, repeats):
    def build():
        return ffn.OcTree.build_from_silhouettes(scene, depth, center, scale, footprint=footprint)
    tree = build() if repeats > 1 else None               # warm-up (none for a single build)
    device, wall, calls = [], [], 0
    for _ in range(repeats):
        torch.cuda.synchronize()
        start = time.perf_counter()
        with EntryPointTimer() as timer:
            tree = build()
        torch.cuda.synchronize()
        wall.append(1e3 * (time.perf_counter() - start))
        device.append(timer.device_ms)
        calls = timer.calls
    case = {"leaves": tree.num_leaves, "entry_point_calls": calls,
            "entry_points_device_ms": min(device), "build_wall_ms": min(wall),
            "timed_builds": repeats}
    return case, tree


def levels_of_box(scene, depth, center, scale, start_level=4):
    """Candidates and survivors per level, through the loop the method runs."""
    images_u8 = torch.from_numpy(np.ascontiguousarray(scene.images)).cuda()
    proj = torch.from_numpy(ffn.projection_matrices(scene.cameras)).cuda()
    mask = (images_u8[..., 3] >= 128).to(torch.float32)
    mask_u8 = torch.nn.functional.max_pool2d(mask[:, None], 3, stride=1,
                                             padding=1)[:, 0].to(torch.uint8).contiguous()
    trace = []
    ffn.OcTree._carve_box_levels(images_u8, mask_u8, proj, center, scale, depth, 128, 0, 2, 1.0,
                                 min(start_level, depth - 1), 1 << 20, trace=trace)
    return [{"level": k, "candidates": c, "survivors": s} for k, c, s in trace]


def bit_count(bits):
    words = bits.to(torch.int64) & 0xffffffff
    return sum(int(((words >> shift) & 1).sum().item()) for shift in range(32))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--repeats", type=int, default=5)
    parser.add_argument("--depths", type=int, nargs="*", default=[8, 10])
    parser.add_argument("--box-only-depths", type=int, nargs="*", default=[11])
    parser.add_argument("--camera-counts", type=int, nargs="+", default=[8, 120])
    parser.add_argument("--size", type=int, default=400)
    parser.add_argument("--truth-depth", type=int, default=9)
    parser.add_argument("--fit-depth", type=int, default=8)
    parser.add_argument("--skip-quality", action="store_true")
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
               "defaults": "alpha_threshold 0.5, dilate 1, max_misses 0, min_views 2, "
                           "cell_opacity 0.5, no merging, start_level 4, batches of 2^20",
               "repeats": args.repeats, "rocprofv3_kernel_times": "not collected", "cases": []}

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(results, indent=1) + "\n")

    for count in args.camera_counts:
        scene = argparse.Namespace(images=images[:count], cameras=cameras[:count],
                                   color_space="RGB")
        for depth in list(args.depths) + list(args.box_only_depths):
            case = {"depth": depth, "cameras": count, "finest_cells": 8 ** (depth - 1)}
            try:
                box, box_tree = build_case(scene, depth, center, scale, "box", args.repeats)
            except (RuntimeError, MemoryError) as error:         # out of memory: recorded as such
                case["box"] = "did not fit: %s" % str(error).splitlines()[0][:200]
                results["cases"].append(case)
                continue
            grey = (box_tree.leaf_data()[:, :3] == np.float32(0.5)).all(1)
            box["share_of_leaves_that_start_grey"] = float(grey.mean())
            box["levels"] = levels_of_box(scene, depth, center, scale)
            case["box"] = box
            if depth in args.depths:
                point, point_tree = build_case(scene, depth, center, scale, "point", args.repeats)
                case["point"] = point
                extra = np.setdiff1d(box_tree.state_dict["leaf_index"],
                                     point_tree.state_dict["leaf_index"])
                lost = np.setdiff1d(point_tree.state_dict["leaf_index"],
                                    box_tree.state_dict["leaf_index"])
                case["box_leaves_that_point_lacks"] = int(len(extra))
                case["point_leaves_that_box_lacks"] = int(len(lost))
                del point_tree
            del box_tree
            results["cases"].append(case)
            print(json.dumps(case), flush=True)
            torch.cuda.empty_cache()
            write()
    if not args.skip_quality:
        train_n = num_cameras - HELD_OUT
        train = quiet(ffn.ImageDataset, "train", images[:train_n], bounds, cameras[:train_n], 8,
                      device="cuda")
        held = quiet(ffn.ImageDataset, "val", images[train_n:], bounds, cameras[train_n:], 8,
                     device="cuda")
        experiment = {"depth": args.fit_depth, "train_cameras": train_n,
                      "held_out_cameras": HELD_OUT, "fit_steps": FIT_STEPS}
        for footprint in ("point", "box"):
            carved = ffn.OcTree.build_from_silhouettes(train, args.fit_depth, center, scale,
                                                       footprint=footprint)

            def volume(tree):
                return lambda starts, dirs: tree.render_volume(starts, dirs).color
            entry = {"leaves": carved.num_leaves,
                     "psnr_as_built": psnr_all_pixels(volume(carved), held, center)}
            fitted, log = ffn.fit_octree(carved, train, None, num_steps=FIT_STEPS, verbose=False)
            entry["psnr_after_fit_octree"] = psnr_all_pixels(volume(fitted), held, center)
            entry["fit_loss_first_last"] = [log[0].loss, log[-1].loss]
            experiment[footprint] = entry
            print(json.dumps({footprint: entry}), flush=True)
        results["held_out_psnr"] = experiment
        write()
        del train, held
        torch.cuda.empty_cache()
        import skip_training_demo as protocol
        scene = protocol.make_scene(protocol.parse_args([]), torch.device("cuda:0"))
        analytic = scene.analytic.bits
        occupancy = {"analytic_bits": bit_count(analytic), "resolution": 128, "depth": 8}
        for dilate in (0, 1):
            for footprint in ("point", "box"):
                grid = ffn.OccupancyGrid.from_silhouettes(scene.train, resolution=128, depth=8,
                                                          dilate=dilate, footprint=footprint)
                lacking = bit_count(analytic & ~grid.bits)
                occupancy["%s_dilate_%d" % (footprint, dilate)] = {
                    "bits": bit_count(grid.bits), "bits_of_the_analytic_grid_it_lacks": lacking,
                    "share_of_the_analytic_grid_it_lacks": lacking / max(bit_count(analytic), 1)}
        results["occupancy_bits"] = occupancy
        print(json.dumps(occupancy), flush=True)
    write()
    return 0


if __name__ == "__main__":
    sys.exit(main())
