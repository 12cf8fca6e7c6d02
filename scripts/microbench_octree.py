"""Microbenchmark of the K12 octree path: surface-point extraction, build_from_samples and query
at 1 M and 16 M points, depth 8, min_leaf_size 4 (voxelize_model.py's defaults).

Reports per size the wall time (synchronised, best of ``--repeats`` after one warm-up call) of
the three calls and, for each C-ABI entry point they make, the bytes it has to move (inputs read
+ outputs written once; the binary searches of the structure step and the gathers of the leaf
means re-read data through the caches and are not counted), so that the achieved fraction of HBM
bandwidth can be read off against kernel times.

    python scripts/microbench_octree.py [--sizes 1048576 16777216] [--repeats 3] [--out result.json]

Kernel times come from a separate profiled run of the same script under
``rocprofv3 --kernel-trace --stats`` (a run of its own: no counters, no other tracing).
"""

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fourier_feature_nets_amd as ffn  # noqa: E402
from fourier_feature_nets_amd import ops  # noqa: E402


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


def cloud(n, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    pos = (torch.rand((n, 3), device="cuda", generator=gen) * 2 - 1) ** 5   # dense centre
    return pos.contiguous(), torch.rand((n, 3), device="cuda", generator=gen)


def bytes_moved(n, leaves, nodes, depth, kept):
    scan = lambda m: 2 * m + 4 * m          # flags read twice, offsets written
    return {
        "ffn_octree_surface_points": n * (4 + 4 + 12 + 12 + 12) + n + scan(n) + n * 5 + kept * 24,
        "ffn_octree_path_codes": n * 12 + n * 4,
        "ffn_octree_structure": n * (4 + 8) + n * (8 + 4 + 8) + n * 8 + n + scan(n) + n * 13
                                + leaves * 20,
        "ffn_octree_interior_nodes": leaves * 8 + leaves * (depth - 1) * (1 + 6 + 5) + nodes * 8,
        "ffn_octree_leaf_means": n * (8 + 12) + leaves * (12 + 12),
        "ffn_octree_query": n * 12 + n * 8,
    }


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--sizes", type=int, nargs="+", default=[1 << 20, 1 << 24])
    parser.add_argument("--depth", type=int, default=8)
    parser.add_argument("--min-leaf-size", type=int, default=4)
    parser.add_argument("--repeats", type=int, default=3)
    parser.add_argument("--out")
    args = parser.parse_args()
    results = {"device": torch.cuda.get_device_name(0), "depth": args.depth,
               "min_leaf_size": args.min_leaf_size, "sizes": {}}
    for n in args.sizes:
        pos, data = cloud(n, n)
        gen = torch.Generator(device="cuda").manual_seed(1)
        alpha = torch.rand((n,), device="cuda", generator=gen)
        depth = torch.rand((n,), device="cuda", generator=gen) * 4
        dirs = torch.nn.functional.normalize(pos, dim=1).contiguous()
        surf_ms, (_, _, count) = wall(lambda: ops.octree_surface_points(
            alpha, depth, pos, dirs, 0.3, data), args.repeats)
        build_ms, tree = wall(lambda: ffn.OcTree.build_from_samples(
            pos, args.depth, args.min_leaf_size, data), args.repeats)
        query_ms, answers = wall(lambda: tree.query(pos * 0.9), args.repeats)
        codes = ops.octree_path_codes(pos, (0.0, 0.0, 0.0), 1.0, args.depth)
        sort_ms, _ = wall(lambda: torch.sort(codes, stable=True), args.repeats)
        nodes = len(tree) - tree.num_leaves
        results["sizes"][str(n)] = {
            "surface_points_wall_ms": surf_ms, "surface_points_kept": int(count.item()),
            "build_wall_ms": build_ms, "of_which_key_sort_wall_ms": sort_ms,
            "query_wall_ms": query_ms, "query_hits": int((answers >= 0).sum().item()),
            "leaves": tree.num_leaves, "interior_nodes": nodes,
            "bytes_moved": bytes_moved(n, tree.num_leaves, nodes, args.depth, int(count.item())),
        }
        del tree, pos, data, alpha, depth, dirs, codes, answers
        torch.cuda.empty_cache()
    line = json.dumps(results, indent=1)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
