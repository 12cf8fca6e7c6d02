"""Microbenchmark of K22, the mesh surface sampler, and of the octree build it feeds.

The mesh is ``procedural_torus()`` (4096 triangles, a 256 x 256 texture), normalised and flipped as
``OcTree.build_from_triangles`` does it.  Recorded, nothing asserted:

* device time (events, best of ``--repeats`` after a warm-up call) of ``ops.mesh_sample`` alone at
  ``N = 2^20`` (the samples of the default depth 8, ``min_leaf_size`` 4) and ``N = 2^26`` (depth 10),
  and the effective write bandwidth at the 24 bytes a sample stores (positions and colours; the
  reads -- offsets, 4096 triangles, the texture -- stay in cache and are not counted);
* the whole of ``OcTree.build_from_triangles`` at depth 8 and 10: wall time between two device
  synchronisations, device time between two events around the call (host gaps included), and the
  share of the latter that is K22;
* at ``2^20``, whether the kernel's output equals the numpy restatement
  (``tests/mesh_reference.py``) bit for bit, and the restatement's wall time on the host -- context
  for the reader, not a comparison of like with like (the reference's own sampler is numba).

    python scripts/microbench_mesh_octree.py [--repeats 5] [--out result.json]
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
from scripts.microbench_octree_refine import wall_ms  # noqa: E402
from scripts.microbench_octree_render import device_ms  # noqa: E402
from tests import mesh_reference  # noqa: E402

BYTES_PER_SAMPLE = 24
MIN_LEAF_SIZE = 4
DEFAULT_OUT = os.path.join(ROOT, "profiles", "r20_mesh_octree_microbench.json")


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--repeats", type=int, default=5)
    parser.add_argument("--depths", type=int, nargs="+", default=[8, 10])
    parser.add_argument("--out", default=DEFAULT_OUT)
    args = parser.parse_args()
    vertices, triangles, uvs, texture = ffn.procedural_torus()
    points = ffn.normalize_points(vertices, (0, 1, 0))
    flipped = np.ascontiguousarray(texture[::-1])
    dev = torch.device("cuda")
    on_device = [torch.from_numpy(np.ascontiguousarray(a)).to(dev)
                 for a in (points, triangles, uvs, flipped)]
    results = {"device": torch.cuda.get_device_name(0),
               "mesh": "procedural_torus(): %d vertices, %d triangles, texture %s"
                       % (len(vertices), len(triangles), "x".join(map(str, texture.shape))),
               "min_leaf_size": MIN_LEAF_SIZE, "repeats": args.repeats,
               "bytes_per_sample": BYTES_PER_SAMPLE,
               "rocprofv3_kernel_times": "not collected",
               "reference_numba_sampler": "not run (numba is not installed)", "cases": []}
    for depth in args.depths:
        n = 8 ** (depth - 2) * MIN_LEAF_SIZE
        counts = ffn.triangle_counts(points, triangles, n, seed=0)
        offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        offsets_dev = torch.from_numpy(offsets).to(dev)
        tensors = (on_device[0], on_device[1], on_device[2], offsets_dev, on_device[3])
        # (ops.mesh_sample reads the ids, UVs and offsets back to check them: timed apart, the
        # launch alone and the wrapper with its checks)
        positions = torch.empty((n, 3), dtype=torch.float32, device=dev)
        colors = torch.empty((n, 3), dtype=torch.float32, device=dev)
        height, width, channels = flipped.shape

        def launch():
            ops._call("ffn_mesh_sample", ops._dev(tensors[0]), ops.c_i64(len(points)),
                      ops._dev(tensors[1], torch.int32), ops.c_i64(len(triangles)),
                      ops._dev(tensors[2]), ops._dev(tensors[3], torch.int32), ops.c_i64(n),
                      ops._dev(tensors[4], torch.uint8), ops.c_i(height), ops.c_i(width),
                      ops.c_i(channels), ops._dev(positions), ops._dev(colors), ops._dev(None))
        kernel_ms = device_ms(launch, args.repeats)
        wrapper_ms = wall_ms(lambda: ops.mesh_sample(*tensors), args.repeats)
        case = {"depth": depth, "samples": n, "largest_triangle_count": int(counts.max()),
                "mesh_sample_device_ms": kernel_ms,
                "mesh_sample_write_GBps": BYTES_PER_SAMPLE * n / (kernel_ms * 1e-3) / 1e9,
                "ops_mesh_sample_wall_ms_with_host_checks": wrapper_ms}
        if n <= 1 << 20:
            start = time.perf_counter()
            want_positions, want_colors, _ = mesh_reference.mesh_sample(points, triangles, uvs,
                                                                        counts, flipped)
            case["numpy_restatement_host_wall_ms"] = 1e3 * (time.perf_counter() - start)
            case["equals_numpy_restatement_bit_for_bit"] = bool(
                np.array_equal(positions.cpu().numpy().view(np.uint32),
                               want_positions.view(np.uint32))
                and np.array_equal(colors.cpu().numpy().view(np.uint32),
                                   want_colors.view(np.uint32)))
        del positions, colors
        torch.cuda.empty_cache()

        def build():
            return ffn.OcTree.build_from_triangles(vertices, triangles, uvs, texture, depth,
                                                   MIN_LEAF_SIZE)
        tree = build()
        case["leaves"] = tree.num_leaves
        del tree
        case["build_from_triangles_wall_ms"] = wall_ms(build, args.repeats)
        case["build_from_triangles_device_ms"] = device_ms(build, args.repeats)
        case["mesh_sample_share_of_build_device_time"] = (kernel_ms
                                                          / case["build_from_triangles_device_ms"])
        results["cases"].append(case)
        torch.cuda.empty_cache()
    line = json.dumps(results, indent=1)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
