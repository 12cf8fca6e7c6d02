"""Microbenchmark of K30, ``OcTree.extract_mesh``: the stages of the extraction next to two things
the same tree already does, for scale.

The trees are those of ``scripts/microbench_octree_density.py``: the density trees of the voxel
radiance field with an opaque ball (``OcTree.build_from_model``) at ``--depths``.  In one process,
best of ``--repeats`` after a warm-up call, per depth:

* the whole ``extract_mesh`` (surface nets; ``--alpha-threshold`` defaults to the 0.01 the trees
  were built with: over one finest side the ball's opacity is 0.17 at depth 8 and 0.05 at depth 10),
  wall time, synchronised, with the vertex and triangle counts and the number of candidates and
  chunks;
* its stages between device events: K30a (opacities and flags), the candidate scan (integer
  plumbing in torch, one read-back), K30b over all chunks (one read-back per chunk), the sort of the
  keys with its payload (``torch.sort``), K30c (vertex attributes), K30d (face flags, scan, one
  read-back, faces and their status read-back);
* ``ops.octree_neighbors`` (K20a) on the same tree and one 400x400 ``render_volume`` frame of
  ``tests/golden/scene16.npz``.

Nothing here asserts a time, and nothing is tuned after the result.  Kernel times under rocprofv3
are not collected.  The result is written after every section, so that a run that is cut short
leaves what it had.

    python scripts/microbench_octree_mesh.py [--repeats 3] [--out profiles/r28_octree_mesh_microbench.json]

``--out`` defaults to ``profiles/r28_octree_mesh_microbench.json``, the recorded run.
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
from scripts.microbench_octree_render import SAMPLES, SIDE, device_ms  # noqa: E402
from scripts.microbench_octree_walk import SCENE, make_sampler, opaque_ball, wall  # noqa: E402


def stages(tree, threshold, batch_size, repeats):
    """The device time of every stage of ``extract_mesh``, on the arrays the stage before left."""
    depth, num = tree.depth, tree.num_leaves
    side = float(np.float32(2.0) * np.float32(tree.scale) / np.float32(1 << (depth - 1)))
    nodes, leaves = tree._on_device("node_index"), tree._on_device("leaf_index")
    rows = tree._colors_on_device()
    out = {}
    out["k30a_solid_device_ms"] = device_ms(
        lambda: ops.octree_mesh_solid(rows, 3, None, num, side, threshold, rows.device), repeats)
    flags, alpha = ops.octree_mesh_solid(rows, 3, None, num, side, threshold, rows.device)
    out["candidate_scan_device_ms"] = device_ms(
        lambda: ops.octree_mesh_candidate_offsets(leaves, flags, depth), repeats)
    offsets, total, _ = ops.octree_mesh_candidate_offsets(leaves, flags, depth)
    out["solid_leaves"] = int(flags.sum().item())
    out["candidates"] = total
    out["chunks"] = (total + batch_size - 1) // batch_size

    def candidates():
        return [ops.octree_mesh_candidates(nodes, leaves, flags, offsets, first,
                                           min(batch_size, total - first), depth)
                for first in range(0, total, batch_size)]
    out["k30b_candidates_device_ms"] = device_ms(candidates, repeats)
    keys, masks, samples = [torch.cat(p) for p in zip(*candidates())]

    def sort():
        sorted_keys, order = torch.sort(keys)
        return sorted_keys, masks[order].contiguous(), samples[order].contiguous()
    out["sort_device_ms"] = device_ms(sort, repeats)
    keys, masks, samples = sort()
    out["k30c_vertices_device_ms"] = device_ms(
        lambda: ops.octree_mesh_vertices(keys, masks, samples, alpha, rows, (0, 1, 0), depth,
                                         tree.scale, (0.0, 0.0, 0.0), threshold, True), repeats)
    out["k30d_faces_device_ms"] = device_ms(lambda: ops.octree_mesh_faces(keys, masks, depth),
                                            repeats)
    return out


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--repeats", type=int, default=3)
    parser.add_argument("--depths", type=int, nargs="+", default=[8, 10])
    parser.add_argument("--alpha-threshold", type=float, default=0.01)
    parser.add_argument("--batch-size", type=int, default=1 << 22)
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles",
                                                      "r28_octree_mesh_microbench.json"))
    args = parser.parse_args()

    def write(results):
        line = json.dumps(results, indent=1)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(line + "\n")
        return line

    scene = dict(np.load(SCENE))
    model = opaque_ball()
    sampler = make_sampler(scene, [0], SIDE, SAMPLES)
    results = {"device": torch.cuda.get_device_name(0), "model": "Voxels(64), opaque ball r=0.45",
               "precision": "f32 (no matrix work on this path)",
               "rocprofv3_kernel_times": "not collected", "frame": [SIDE, SIDE],
               "repeats": args.repeats, "alpha_threshold": args.alpha_threshold,
               "placement": "surface_nets", "batch_size": args.batch_size, "cases": [],
               "complete": False}
    for depth in args.depths:
        tree = ffn.OcTree.build_from_model(model, depth, alpha_threshold=0.01)
        case = {"depth": depth, "leaves": tree.num_leaves}
        results["cases"].append(case)
        ms, mesh = wall(lambda: tree.extract_mesh(args.alpha_threshold,
                                                  batch_size=args.batch_size), args.repeats)
        case["extract_mesh_wall_ms"] = ms
        case["vertices"], case["triangles"] = len(mesh.vertices), len(mesh.triangles)
        del mesh
        write(results)
        case["stages"] = stages(tree, args.alpha_threshold, args.batch_size, args.repeats)
        write(results)
        nodes, leaves = tree._on_device("node_index"), tree._on_device("leaf_index")
        case["neighbors_k20a_device_ms"] = device_ms(lambda: ops.octree_neighbors(nodes, leaves),
                                                     args.repeats)
        shift = torch.tensor(tree.center, dtype=torch.float32, device="cuda")
        starts = (sampler.starts - shift).contiguous()
        directions = sampler.directions.contiguous()
        case["render_volume_frame_device_ms"] = device_ms(
            lambda: tree.render_volume(starts, directions), args.repeats)
        write(results)
        del tree, nodes, leaves
        torch.cuda.empty_cache()
    results["complete"] = True
    print(write(results))
    return 0


if __name__ == "__main__":
    sys.exit(main())
