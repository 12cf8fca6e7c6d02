"""Microbenchmark of K25, occupancy bits from an octree's leaves (``OccupancyGrid.from_octree``).

Trees: the torus dataset of ``scripts/make_mesh_npz.py`` (made in memory as
``microbench_octree_carve.py`` makes it: 120 cameras of 400 x 400), carved at depth 8 and 10 from
all cameras with the defaults; and a root-only tree, the widest footprint there is.  Grids: G = 128
and 256 over the dataset's bounds; the root-only tree at G = 256 over its own cube.  Recorded per
case, nothing asserted, nothing tuned afterwards:

* the device time of the K25 entry point alone (events, best of ``--repeats`` after a warm-up;
  buffers allocated beforehand, no dilation; the entry point reads its row count back, so the
  time includes that one synchronisation), and the wall time of the whole ``from_octree``
  (dilate 1, the default);
* the leaves, the rows of the second kernel and the bits set, undilated and dilated;
* for context, in the same process, the composition from what was public before K25:
  ``tree.query(OccupancyGrid.cell_centres(...))`` -> ``from_logits`` without dilation: its wall
  time, and how many of K25's undilated bits it lacks.  It answers a different, weaker question
  (is the cell's CENTRE inside a leaf), so no ratio is promised: the lacking bits are the point.

    python scripts/microbench_occupancy_octree.py [--repeats 5] [--out result.json]
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
from scripts.microbench_octree_carve import torus_dataset  # noqa: E402
from scripts.microbench_octree_refine import wall_ms  # noqa: E402
from scripts.microbench_octree_render import device_ms  # noqa: E402

DEFAULT_OUT = os.path.join(ROOT, "profiles", "r23_occupancy_octree_microbench.json")


def bit_count(bits):
    words = bits.to(torch.int64) & 0xffffffff
    return sum(int(((words >> shift) & 1).sum().item()) for shift in range(32))


def entry_point_ms(tree, center, lo, size, g, repeats):
    """The K25 entry point alone, into preallocated buffers -> (ms, rows, bits tensor)."""
    dev = tree._dev()
    ids = tree._on_device("leaf_index")
    leaves = ids.shape[0]
    words = (g ** 3 + 31) // 32
    bits = torch.empty((words,), dtype=torch.int32, device=dev)
    plan = torch.empty((leaves, 4), dtype=torch.int32, device=dev)
    offsets = torch.empty((leaves,), dtype=torch.int32, device=dev)
    tiles = torch.empty(((leaves + 4095) // 4096,), dtype=torch.int32, device=dev)
    total = torch.empty((1,), dtype=torch.int64, device=dev)

    def launch():
        ops._call("ffn_occupancy_from_octree", ops._dev(ids, torch.int64), ops.c_i64(leaves),
                  ops.c_f(tree.scale), ops._host3(center), ops._dev(None), ops.c_i(4), ops.c_i(3),
                  ops.c_f(0.0), ops.c_i(0), ops._host3(lo), ops._host3(size), ops.c_i(g),
                  ops.c_i(0), ops.c_i(0), ops._dev(plan, torch.int32), ops._dev(offsets, torch.int32),
                  ops._dev(tiles, torch.int32), ops._dev(total, torch.int64), ops._dev(None),
                  ops._dev(bits, torch.int32))
    ms = device_ms(launch, repeats)
    return ms, int(total.item()), bits


def case(name, tree, center, bounds, g, repeats):
    dev = tree._dev()
    lo, size = ffn.OccupancyGrid.box_of(bounds)
    ms, rows, bits = entry_point_ms(tree, center, lo, size, g, repeats)
    out = {"tree": name, "G": g, "leaves": tree.num_leaves, "rows": rows,
           "k25_entry_point_device_ms": ms, "bits_undilated": bit_count(bits)}

    def whole():
        return ffn.OccupancyGrid.from_octree(tree, bounds, g, center=center)
    out["from_octree_wall_ms_dilate_1"] = wall_ms(whole, repeats)
    out["bits_dilate_1"] = bit_count(whole().bits)

    shift = torch.tensor(center, dtype=torch.float32, device=dev)

    def composition():
        centres = ffn.OccupancyGrid.cell_centres(bounds, g, dev)
        hit = tree.query(centres - shift) >= 0
        logits = torch.full((g ** 3, 4), -100.0, device=dev)
        logits[hit, 3] = 100.0
        return ffn.OccupancyGrid.from_logits(logits, bounds, g, 0.01, dilate=False)
    out["cell_centre_composition_wall_ms"] = wall_ms(composition, repeats)
    sampled = composition().bits
    out["cell_centre_composition_bits"] = bit_count(sampled)
    out["k25_bits_the_composition_lacks"] = bit_count(bits & ~sampled)
    out["composition_bits_k25_lacks"] = bit_count(sampled & ~bits)
    return out


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--repeats", type=int, default=5)
    parser.add_argument("--depths", type=int, nargs="+", default=[8, 10])
    parser.add_argument("--resolutions", type=int, nargs="+", default=[128, 256])
    parser.add_argument("--cameras", type=int, default=120)
    parser.add_argument("--size", type=int, default=400)
    parser.add_argument("--truth-depth", type=int, default=9)
    parser.add_argument("--out", default=DEFAULT_OUT)
    args = parser.parse_args()
    truth, images, cameras, bounds = torus_dataset(args.cameras, args.size, args.truth_depth)
    center, scale = truth.center, truth.scale
    results = {"device": torch.cuda.get_device_name(0),
               "dataset": "procedural_torus() at depth %d, %d cameras of %d x %d, first-hit frames; "
                          "carved from all cameras, defaults, no merging"
                          % (args.truth_depth, args.cameras, args.size, args.size),
               "cube": {"center": list(center), "scale": scale},
               "box": "the dataset's bounds, [-1, 1]^3; the root-only tree's own cube",
               "repeats": args.repeats, "rocprofv3_kernel_times": "not collected", "cases": []}
    scene = argparse.Namespace(images=images, cameras=cameras, color_space="RGB")
    for depth in args.depths:
        tree = ffn.OcTree.build_from_silhouettes(scene, depth, center, scale)
        for g in args.resolutions:
            row = case("carved depth %d" % depth, tree, center, bounds, g, args.repeats)
            results["cases"].append(row)
            print(json.dumps(row), flush=True)
            torch.cuda.empty_cache()
        del tree
    root = ffn.OcTree(1.0, np.zeros(0, np.int64), np.zeros(1, np.int64))
    root._device = torch.device("cuda")
    row = case("root only", root, (0.0, 0.0, 0.0), np.diag([2.0, 2.0, 2.0, 1.0]), 256, args.repeats)
    results["cases"].append(row)
    print(json.dumps(row), flush=True)
    line = json.dumps(results, indent=1)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
