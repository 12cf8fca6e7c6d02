"""Microbenchmark of K18: spherical-harmonic leaves in a baked octree.

The tree and the rays are those of ``scripts/microbench_octree_density.py``: the depth-8 density
tree of the voxel radiance field with an opaque ball (``OcTree.build_from_model``) and the 400x400
rays of the first training camera of ``tests/golden/scene16.npz``.  In one process:

* wall and device time of ``render_volume`` of the plain tree (K15) and of the degree-1 and
  degree-2 SH trees ``bake_sh`` makes of the same model (K18a), and their ratios to K15;
* wall time of ``bake`` and of ``bake_sh`` (64 views) on that tree;
* for a model WITH a view direction -- a small NeRF trained for ``--train-steps`` steps on the
  scene, or, when that fails, a randomly initialised one; ``view_model`` says which -- a density
  tree of ``--view-depth`` built from it and baked three ways (one fixed view, SH degree 1, SH
  degree 2), each against the model's own render over ``--psnr-cameras`` cameras: PSNR over the
  pixels where the model's alpha is >= 0.99, and over all valid pixels.

Nothing here asserts a time or a PSNR.  Kernel times under rocprofv3 are not collected here.

    python scripts/microbench_octree_sh.py [--repeats 3] [--out result.json]
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
from scripts.microbench_octree_render import SAMPLES, SIDE, device_ms  # noqa: E402
from scripts.microbench_octree_walk import (SCENE, make_sampler, opaque_ball,  # noqa: E402
                                            render_valid, wall)


def psnr(err):
    return float(-10 * np.log10(max(float(err.mean()), 1e-12))) if err.size else None


def view_model(steps):
    """-> (model, label): a small NeRF, trained briefly when training works here."""
    torch.manual_seed(0)
    np.random.seed(0)
    model = ffn.NeRF(4, 128, 5, 6, 2, 3, [2], True).to("cuda")
    if steps <= 0:
        return model, "NeRF(4, 128), randomly initialised"
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            train = ffn.ImageDataset.load(SCENE, "train", 64, True, False, None, device="cuda")
            val = ffn.ImageDataset.load(SCENE, "val", 64, True, False, None, device="cuda")
            ffn.Raycaster(model).fit(train, val, 1024, 5e-4, steps, 0, steps, 0.1, 25000, 0.0, [])
        return model, "NeRF(4, 128), trained for %d steps of 1024 rays on scene16" % steps
    except Exception as error:      # the label says what the numbers are of
        torch.manual_seed(0)
        model = ffn.NeRF(4, 128, 5, 6, 2, 3, [2], True).to("cuda")
        return model, "NeRF(4, 128), randomly initialised (training failed: %s)" % (error,)


def compare(tree, starts, dirs, want_c, want_a):
    shift = torch.tensor(tree.center, dtype=torch.float32, device="cuda")
    out = tree.render_volume((starts - shift).contiguous(), dirs)
    err = ((out.color - want_c) ** 2).double().cpu().numpy()
    opaque = want_a.cpu().numpy() >= 0.99
    return {"psnr_where_model_alpha_ge_0.99": psnr(err[opaque]), "psnr_all_valid_pixels": psnr(err),
            "mean_abs_alpha_difference": float((out.alpha - want_a).abs().mean().item())}


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--repeats", type=int, default=3)
    parser.add_argument("--depth", type=int, default=8)
    parser.add_argument("--view-depth", type=int, default=7)
    parser.add_argument("--num-views", type=int, default=64)
    parser.add_argument("--psnr-cameras", type=int, default=4)
    parser.add_argument("--train-steps", type=int, default=1000)
    parser.add_argument("--out")
    args = parser.parse_args()
    data = dict(np.load(SCENE))
    n_train = int(data["split_counts"][0])
    cameras = list(range(min(args.psnr_cameras, n_train)))
    sampler = make_sampler(data, cameras, SIDE, SAMPLES)
    index = sampler.valid_index(torch.arange(len(sampler), device="cuda"))
    starts, dirs = sampler.starts[index].contiguous(), sampler.directions[index].contiguous()
    one = index[index < sampler.rays_per_camera]
    o1, d1 = sampler.starts[one].contiguous(), sampler.directions[one].contiguous()

    ball = opaque_ball()
    plain = ffn.OcTree.build_from_model(ball, args.depth)
    results = {"device": torch.cuda.get_device_name(0), "precision": "f32 (no matrix work here)",
               "rocprofv3_kernel_times": "not collected", "frame": [SIDE, SIDE],
               "rays_of_camera_0": int(one.numel()), "repeats": args.repeats,
               "num_views": args.num_views,
               "tree": {"model": "Voxels(64), opaque ball r=0.45", "depth": args.depth,
                        "leaves": plain.num_leaves}, "render_volume": {}, "bake": {}}
    results["bake"]["bake_wall_ms"], _ = wall(lambda: plain.bake(ball), args.repeats)
    trees = {"plain_k15": plain}
    for degree in (1, 2):
        ms, tree = wall(lambda: plain.bake_sh(ball, degree, args.num_views), args.repeats)
        results["bake"]["bake_sh_degree_%d_wall_ms" % degree] = ms
        results["bake"]["bake_sh_degree_%d_over_bake" % degree] = ms / results["bake"]["bake_wall_ms"]
        trees["sh_degree_%d" % degree] = tree
    shift = torch.tensor(plain.center, dtype=torch.float32, device="cuda")
    o = (o1 - shift).contiguous()
    for name, tree in trees.items():
        geometry = (o, d1, tree.scale, tree.depth, tree._on_device("node_index"),
                    tree._on_device("leaf_index"))
        entry = {}
        entry["wall_ms"], _ = wall(lambda: tree.render_volume(o, d1), args.repeats)
        if tree.sh_degree is None:
            leaf_data = tree._colors_on_device()
            entry["device_ms"] = device_ms(lambda: ops.octree_render_volume(*geometry, leaf_data),
                                           args.repeats)
        else:
            rows = tree._sh_rows_on_device()
            entry["device_ms"] = device_ms(
                lambda: ops.octree_render_volume_sh(*geometry, rows, tree.sh_degree), args.repeats)
            entry["bytes_per_leaf_row"] = int(rows.shape[1]) * 4
        results["render_volume"][name] = entry
    base = results["render_volume"]["plain_k15"]
    for name in ("sh_degree_1", "sh_degree_2"):
        entry = results["render_volume"][name]
        entry["device_ms_over_k15"] = entry["device_ms"] / base["device_ms"]
        entry["wall_ms_over_k15"] = entry["wall_ms"] / base["wall_ms"]

    model, label = view_model(args.train_steps)
    caster = ffn.Raycaster(model)
    want_c, want_a, _ = render_valid(caster, sampler, index)
    view = {"view_model": label, "depth": args.view_depth, "cameras": cameras,
            "valid_rays": int(index.numel()), "model_samples_per_ray": SAMPLES,
            "pixels_where_model_alpha_ge_0.99": int((want_a >= 0.99).sum().item()), "trees": {}}
    try:
        bare = ffn.OcTree.build_from_model(model, args.view_depth)
        view["leaves"] = bare.num_leaves
        baked = {"one_fixed_view": bare.bake(model),
                 "sh_degree_1": bare.bake_sh(model, 1, args.num_views),
                 "sh_degree_2": bare.bake_sh(model, 2, args.num_views)}
        for name, tree in baked.items():
            view["trees"][name] = compare(tree, starts, dirs, want_c, want_a)
    except ValueError as error:             # a model without density has no tree
        view["error"] = str(error)
    results["view_dependent_model"] = view
    line = json.dumps(results, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
