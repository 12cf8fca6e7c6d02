"""Microbenchmark of K21, refining a fitted octree: the per-leaf maximum weight next to the volume
render it shares its walk with, the rebuild from a per-leaf decision, and the experiment the feature
exists for.

The model and the cameras are those of ``scripts/microbench_octree_density.py`` (the voxel radiance
field with an opaque ball, 400x400 rays of scene16's training cameras); the trees are
``OcTree.build_from_model`` at depth 8 and 10.  Per depth:

* device time (events, best of ``--repeats`` after a warm-up call) of ``render_volume`` (K15) and of
  ``leaf_weights`` (K21a, into a zeroed buffer and folding into a buffer that already holds the
  answer) on every ray of camera 0 and on a shuffled 4096-ray batch, in the same process;
* a split of every leaf where the result fits the depth limit (K21b with the sort to code order,
  K12h and the sort back): wall time of ``ops.octree_refine`` and device time of its two entry
  points alone.

The experiment, the held-out protocol of the K17 paragraph (two training and two held-out cameras,
targets the model's own renders): arm A fits the depth-8 tree for ``--fit-steps`` steps; arm B fits
the depth-7 tree for half of them, refines once at the default thresholds and fits for the other
half (``fit_octree_adaptive``, ``rounds=1``).  Leaf counts, the share pruned, the step time and the
held-out PSNR (all pixels, and where the model is opaque) before and after.  Nothing here asserts a
time or a PSNR, and nothing is tuned after the result.

    python scripts/microbench_octree_refine.py [--repeats 5] [--out result.json]
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
from fourier_feature_nets_amd import octree_fit, ops  # noqa: E402
from scripts.microbench_octree_fit import ModelTargets, psnr_pair  # noqa: E402
from scripts.microbench_octree_render import SAMPLES, SIDE, device_ms  # noqa: E402
from scripts.microbench_octree_walk import SCENE, make_sampler, opaque_ball  # noqa: E402


def wall_ms(fn, repeats):
    """Best wall time of ``fn`` between two device synchronisations, after one warm-up call."""
    fn()
    best = float("inf")
    for _ in range(repeats):
        torch.cuda.synchronize()
        start = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - start) * 1e3)
    return best


def refine_kernels_ms(leaf_ids, rows, action, repeats):
    """Device time of the two K21b entry points alone.  The ids come in id order, not code order:
    for a split of every leaf that changes which id lands where, not the work that is timed."""
    num, channels = rows.shape
    flags, offsets, tiles = ops._scan_scratch(8 * num, rows.device)
    total = torch.zeros((), dtype=torch.int32, device=rows.device)

    def count():
        ops._call("ffn_octree_refine_count", ops._dev(action, torch.uint8), ops.c_i64(num),
                  ops._dev(flags, torch.uint8), ops._dev(offsets, torch.int32),
                  ops._dev(tiles, torch.int32), ops._dev(total, torch.int32))
    count()
    new = int(total.item())
    ids_out = torch.empty((new,), dtype=torch.int64, device=rows.device)
    rows_out = torch.empty((new, channels), dtype=torch.float32, device=rows.device)
    parent = torch.empty((new,), dtype=torch.int32, device=rows.device)

    def scatter():
        ops._call("ffn_octree_refine_scatter", ops._dev(action, torch.uint8),
                  ops._dev(flags, torch.uint8), ops._dev(offsets, torch.int32),
                  ops._dev(leaf_ids, torch.int64), ops._dev(rows), ops.c_i64(num),
                  ops.c_i(channels), ops.c_i64(new), ops._dev(ids_out, torch.int64),
                  ops._dev(rows_out), ops._dev(parent, torch.int32))
    return {"count_and_scan_device_ms": device_ms(count, repeats),
            "scatter_device_ms": device_ms(scatter, repeats), "new_leaves": new}


def step_ms(log_len, seconds):
    return 1e3 * seconds / max(log_len, 1)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--repeats", type=int, default=5)
    parser.add_argument("--depths", type=int, nargs="+", default=[8, 10])
    parser.add_argument("--fit-cameras", type=int, default=2)
    parser.add_argument("--fit-steps", type=int, default=300)
    parser.add_argument("--out")
    args = parser.parse_args()
    scene = dict(np.load(SCENE))
    n_train = int(scene["split_counts"][0])
    model = opaque_ball()
    caster = ffn.Raycaster(model)
    fit_cameras = list(range(min(args.fit_cameras, n_train - 2)))
    held_out = [n_train - 2, n_train - 1]
    train = ModelTargets(caster, make_sampler(scene, fit_cameras, SIDE, SAMPLES))
    val = ModelTargets(caster, make_sampler(scene, held_out, SIDE, SAMPLES))
    sampler = train.sampler
    per = sampler.rays_per_camera
    results = {"device": torch.cuda.get_device_name(0), "model": "Voxels(64), opaque ball r=0.45",
               "precision": "f32 (no matrix work on this path; bf16x6 not run)",
               "rocprofv3_kernel_times": "not collected", "frame": [SIDE, SIDE],
               "repeats": args.repeats, "targets": "the model's own render (colour * alpha, alpha)",
               "fit_cameras": fit_cameras, "held_out_cameras": held_out, "cases": []}
    limit = ops.octree_max_depth()
    for depth in args.depths:
        tree = ffn.OcTree.build_from_model(model, depth, alpha_threshold=0.01)
        shift = torch.tensor(tree.center, dtype=torch.float32, device="cuda")
        nodes, leaves = tree._on_device("node_index"), tree._on_device("leaf_index")
        geometry = (tree.scale, tree.depth, nodes, leaves)
        data = tree._colors_on_device()
        case = {"depth": depth, "leaves": tree.num_leaves, "rays": {}}
        shuffled = torch.randperm(len(sampler), device="cuda",
                                  generator=torch.Generator(device="cuda").manual_seed(2))[:4096]
        for name, rays in (("camera_0", torch.arange(per, device="cuda")),
                           ("batch_4096", shuffled)):
            o = (sampler.starts[rays] - shift).contiguous()
            d = sampler.directions[rays].contiguous()
            out = torch.zeros((tree.num_leaves,), dtype=torch.float32, device="cuda")

            def fresh():
                out.zero_()
                ops.octree_leaf_weights(o, d, *geometry, data, 4, 3, out=out)
            render_ms = device_ms(lambda: ops.octree_render_volume(o, d, *geometry, data),
                                  args.repeats)
            zero_ms = device_ms(out.zero_, args.repeats)
            fresh_ms = device_ms(fresh, args.repeats)
            folded_ms = device_ms(lambda: ops.octree_leaf_weights(o, d, *geometry, data, 4, 3,
                                                                  out=out), args.repeats)
            case["rays"][name] = {
                "rays": int(rays.numel()), "leaves_with_weight": int((out > 0).sum().item()),
                "render_volume_device_ms": render_ms, "zero_fill_device_ms": zero_ms,
                "leaf_weights_zeroed_device_ms": fresh_ms - zero_ms,
                "leaf_weights_folding_device_ms": folded_ms,
                "leaf_weights_over_render_volume": (fresh_ms - zero_ms) / render_ms}
        if depth + 1 <= limit:
            action = torch.full((tree.num_leaves,), 2, dtype=torch.uint8, device="cuda")
            whole = wall_ms(lambda: ops.octree_refine(leaves, data, action, tree.depth),
                            args.repeats)
            case["split_all"] = dict(refine_kernels_ms(leaves, data, action, args.repeats),
                                     octree_refine_wall_ms=whole)
        else:
            case["split_all"] = "a depth-%d tree cannot split: the walk holds %d levels" % (depth,
                                                                                          limit)
        results["cases"].append(case)
        del tree, data, nodes, leaves
        torch.cuda.empty_cache()

    # the experiment
    steps = args.fit_steps
    arms = {}
    coarse = ffn.OcTree.build_from_model(model, 7, alpha_threshold=0.01)
    fine = ffn.OcTree.build_from_model(model, 8, alpha_threshold=0.01)
    torch.cuda.synchronize()
    start = time.perf_counter()
    fitted, log = ffn.fit_octree(fine, train, None, 4096, num_steps=steps, verbose=False)
    torch.cuda.synchronize()
    arms["A_depth8_plain"] = {
        "steps": steps, "leaves": fine.num_leaves, "psnr_before": psnr_pair(fine, val),
        "psnr_after": psnr_pair(fitted, val), "step_wall_ms": step_ms(len(log),
                                                                      time.perf_counter() - start),
        "loss_first_16": float(np.mean([e.loss for e in log[:16]])),
        "loss_last_16": float(np.mean([e.loss for e in log[-16:]]))}
    # arm B by hand, as fit_octree_adaptive(rounds=1) runs it, to time and score its parts
    torch.cuda.synchronize()
    start = time.perf_counter()
    first, log1 = ffn.fit_octree(coarse, train, None, 4096, num_steps=steps // 2, verbose=False)
    torch.cuda.synchronize()
    first_s = time.perf_counter() - start
    start = time.perf_counter()
    weights = ffn.leaf_weights_over(first, train)
    report, refined = octree_fit.refine_once(first, weights, 0, octree_fit.PRUNE_BELOW,
                                              octree_fit.SPLIT_ABOVE, None)
    torch.cuda.synchronize()
    refine_s = time.perf_counter() - start
    start = time.perf_counter()
    second, log2 = ffn.fit_octree(refined, train, None, 4096, num_steps=steps - steps // 2,
                                  verbose=False)
    torch.cuda.synchronize()
    second_s = time.perf_counter() - start
    arms["B_depth7_refined"] = {
        "steps": [steps // 2, steps - steps // 2], "prune_below": octree_fit.PRUNE_BELOW,
        "split_above": octree_fit.SPLIT_ABOVE, "report": report._asdict(),
        "fraction_pruned": report.dropped / report.leaves_before,
        "measure_and_refine_wall_ms": 1e3 * refine_s,
        "psnr_before": psnr_pair(coarse, val), "psnr_after_first_fit": psnr_pair(first, val),
        "psnr_after_refine": psnr_pair(refined, val), "psnr_after": psnr_pair(second, val),
        "step_wall_ms_before": step_ms(len(log1), first_s),
        "step_wall_ms_after": step_ms(len(log2), second_s),
        "loss_first_16": float(np.mean([e.loss for e in log1[:16]])),
        "loss_last_16": float(np.mean([e.loss for e in log2[-16:]]))}
    # the driver gives the same tree
    driven, _, _ = ffn.fit_octree_adaptive(coarse, train, None, rounds=1, batch_size=4096,
                                           num_steps=steps // 2, verbose=False)
    arms["B_depth7_refined"]["fit_octree_adaptive_gives_the_same_tree"] = bool(
        steps % 2 == 0 and np.array_equal(driven.state_dict["leaf_index"],
                                          second.state_dict["leaf_index"])
        and np.array_equal(driven.leaf_data(), second.leaf_data()))
    results["experiment"] = arms
    line = json.dumps(results, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
