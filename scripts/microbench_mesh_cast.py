"""Microbenchmark of K36 -- rays against a triangle mesh through a Morton-ordered tree -- in the
setting of ``scripts/microbench_mesh_raster.py``: the rays of one 400 x 400 camera against the
procedural torus and the K30 meshes of the opaque ball (surface nets of the depth-8 and depth-10
density trees).

Times, in one process, best of ``--repeats`` after a warm-up call, between device events:

* ``build_mesh_bvh`` (K36a, torch's sort, K36b; it reads the extent of the vertices back once), and
  K36a and K36b on their own;
* the nearest cast (K36c), the farthest cast, ``mesh_spans`` (two casts) and K36d;
* next to them K31's frame of the same mesh from the same camera (``rasterize_mesh``: set-up, scan,
  draw, resolve and its one read-back) and ``OcTree.first_hit`` of the tree the mesh stands for, on
  the same rays.

It also records how far the walk goes: the mean number of nodes visited and triangles tested per
ray, counted by the numpy restatement (tests/mesh_cast_reference.py) on a subsample of
``--counted-rays`` rays, whose hits are asserted to be the device's.

No time is gated and nothing is tuned after the result.

    python scripts/microbench_mesh_cast.py [--out profiles/r34_mesh_cast_microbench.json]
"""

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import fourier_feature_nets_amd as ffn  # noqa: E402
from fourier_feature_nets_amd import mesh as mesh_module  # noqa: E402
from fourier_feature_nets_amd import ops  # noqa: E402
from scripts.microbench_mesh_raster import on_gpu, rig  # noqa: E402
from scripts.microbench_octree_carve import quiet  # noqa: E402
from scripts.microbench_octree_render import device_ms  # noqa: E402
from scripts.microbench_octree_walk import opaque_ball, wall  # noqa: E402

DEFAULT_OUT = os.path.join(ROOT, "profiles", "r34_mesh_cast_microbench.json")


def cast_case(vertices, triangles, colors, camera, sampler, tree, args):
    """One mesh (numpy arrays) under the rays of ``sampler``'s first camera."""
    from tests import mesh_cast_reference as reference
    repeats = args.repeats
    width, height = camera.resolution
    v, t = on_gpu(vertices, "float32"), on_gpu(triangles, "int32")
    c = on_gpu(colors, "float32")
    starts = sampler.starts[:sampler.rays_per_camera].contiguous()
    directions = sampler.directions[:sampler.rays_per_camera].contiguous()
    out = {"vertices": len(vertices), "triangles": len(triangles), "rays": int(starts.shape[0]),
           "leaf_size": args.leaf_size}

    out["build_mesh_bvh_device_ms"] = device_ms(
        lambda: ffn.build_mesh_bvh(v, t, args.leaf_size), repeats)
    out["build_mesh_bvh_wall_ms"] = wall(lambda: ffn.build_mesh_bvh(v, t, args.leaf_size),
                                         repeats)[0]
    bvh = ffn.build_mesh_bvh(v, t, args.leaf_size)
    out["levels"], out["nodes"], out["pad"] = bvh.levels, int(bvh.nodes.shape[0]), bvh.pad
    low, high, _ = mesh_module._finite_extent(v)
    scale = 1024.0 / float((high - low).max())
    out["k36a_boxes_device_ms"] = device_ms(
        lambda: ops.mesh_cast_boxes(v, t, bvh.pad, low, scale), repeats)
    out["k36b_tree_device_ms"] = device_ms(
        lambda: ops.mesh_cast_tree(bvh.boxes, bvh.order, args.leaf_size), repeats)

    mesh = (bvh.nodes, bvh.boxes, bvh.order, v, t)
    out["k36c_nearest_device_ms"] = device_ms(
        lambda: ops.mesh_cast(*mesh, starts, directions, args.leaf_size), repeats)
    out["k36c_farthest_device_ms"] = device_ms(
        lambda: ops.mesh_cast(*mesh, starts, directions, args.leaf_size, 0.0, True), repeats)
    out["mesh_spans_device_ms"] = device_ms(lambda: ffn.mesh_spans(bvh, starts, directions), repeats)
    hit, t_hit, u, w = ops.mesh_cast(*mesh, starts, directions, args.leaf_size)
    out["k36d_shade_device_ms"] = device_ms(
        lambda: ops.mesh_cast_shade(hit, t_hit, u, w, t, c, None, None), repeats)
    out["render_mesh_rays_wall_ms"] = wall(
        lambda: ffn.render_mesh_rays(bvh, starts, directions, colors=c), repeats)[0]
    out["rays_that_hit_share"] = float((hit >= 0).float().mean().item())
    out["k36c_nearest_rays_per_second"] = starts.shape[0] / out["k36c_nearest_device_ms"] * 1e3

    proj = ffn.projection_matrices([camera])[0]
    eye = ffn.eye_positions([camera], (0.0, 0.0, 0.0))[0]
    out["k31_frame_device_ms"] = device_ms(
        lambda: mesh_module.rasterize_mesh(v, t, proj, eye, width, height, c), repeats)
    ids = mesh_module.rasterize_mesh(v, t, proj, eye, width, height, c)[3]
    out["pixels_whose_triangle_differs_from_k31_share"] = float((ids != hit).float().mean().item())
    out["k36c_nearest_over_k31_frame"] = out["k36c_nearest_device_ms"] / out["k31_frame_device_ms"]

    if tree is not None:
        shift = torch.tensor(tree.center, dtype=torch.float32, device="cuda")
        moved = (starts - shift).contiguous()
        out["tree"] = {"leaves": tree.num_leaves, "depth": tree.depth,
                       "first_hit_device_ms": device_ms(lambda: tree.first_hit(moved, directions),
                                                        repeats),
                       "spans_device_ms": device_ms(lambda: tree.spans(moved, directions, 0.0, 0.0),
                                                    repeats)}
        out["k36c_nearest_over_octree_first_hit"] = (out["k36c_nearest_device_ms"]
                                                     / out["tree"]["first_hit_device_ms"])

    # how far the walk goes, counted by the restatement on a subsample of the rays
    rows = np.random.default_rng(0).choice(starts.shape[0], min(args.counted_rays, starts.shape[0]),
                                           replace=False)
    rows.sort()
    host = reference.build(vertices, triangles, args.leaf_size, pad=bvh.pad,
                           order=bvh.order.cpu().numpy())
    some = torch.from_numpy(rows).cuda()
    found = reference.cast(host, vertices, triangles, starts[some].cpu().numpy(),
                           directions[some].cpu().numpy(), counts=True)
    assert np.array_equal(found[0], hit[some].cpu().numpy())
    assert np.array_equal(found[1].view(np.uint32), t_hit[some].cpu().numpy().view(np.uint32))
    out["counted_rays"] = len(rows)
    out["mean_nodes_visited_per_ray"] = float(found[4].mean())
    out["most_nodes_visited_by_a_ray"] = int(found[4].max())
    out["mean_triangles_tested_per_ray"] = float(found[5].mean())
    out["most_triangles_tested_by_a_ray"] = int(found[5].max())
    return out


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--repeats", type=int, default=5)
    parser.add_argument("--depths", type=int, nargs="*", default=[8, 10])
    parser.add_argument("--size", type=int, default=400)
    parser.add_argument("--leaf-size", type=int, default=4)
    parser.add_argument("--torus-depth", type=int, default=8)
    parser.add_argument("--counted-rays", type=int, default=1000)
    parser.add_argument("--out", default=DEFAULT_OUT)
    args = parser.parse_args()
    results = {"device": torch.cuda.get_device_name(0), "frame": [args.size, args.size],
               "repeats": args.repeats, "precision": "f32 and integers (no matrix work on this path)",
               "rocprofv3_kernel_times": "not collected", "cases": [], "complete": False}

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(results, indent=1) + "\n")

    camera = rig(8, args.size)[0]
    bounds = np.diag([2, 2, 2, 1]).astype(np.float32)
    sampler = quiet(ffn.RaySampler, bounds, [camera], 8, device="cuda")
    torus = ffn.procedural_torus()
    points = ffn.normalize_points(torus[0])
    grey = np.random.default_rng(1).uniform(0, 1, (len(points), 3)).astype(np.float32)
    case = {"mesh": "procedural_torus(), normalised; the tree is its depth-%d colour tree (K22)"
                    % args.torus_depth}
    case.update(cast_case(points, torus[1], grey, camera, sampler,
                          ffn.OcTree.build_from_triangles(*torus, args.torus_depth, 4), args))
    results["cases"].append(case)
    print(json.dumps(case), flush=True)
    write()
    model = opaque_ball() if args.depths else None
    for depth in args.depths:
        tree = ffn.OcTree.build_from_model(model, depth, alpha_threshold=0.01)
        surface = tree.extract_mesh(0.01)
        case = {"mesh": "extract_mesh(0.01, surface_nets) of the depth-%d density tree" % depth}
        case.update(cast_case(surface.vertices, surface.triangles, surface.colors, camera, sampler,
                              tree, args))
        results["cases"].append(case)
        print(json.dumps(case), flush=True)
        write()
        del tree, surface
        torch.cuda.empty_cache()
    results["complete"] = True
    write()
    return 0


if __name__ == "__main__":
    sys.exit(main())
