"""Microbenchmark of K24, colouring leaves from the cameras that can see them
(``OcTree.visible_votes`` / ``color_from_images`` / ``build_from_silhouettes(color="visible")``), and
the experiment it exists for.

The dataset is the one ``scripts/make_mesh_npz.py`` writes for the procedural torus, made in memory
as ``scripts/microbench_octree_carve.py`` makes it (120 cameras of 400 x 400).  Recorded, nothing
asserted, nothing tuned afterwards:

* per depth (8 and 10): the tree carved from all 120 cameras with the defaults, and per camera count
  (the first 8, all 120) the device time of the K24 entry point over every (leaf, camera) pair
  (events, best of ``--repeats`` after a warm-up), leaves and pairs per second, the share of the
  pairs rejected before the walk (behind the camera, off the image, background pixel) and the
  share that ends visible;
* next to it, in the same process, THE SAME QUESTION COMPOSED FROM THE PUBLIC OPS that were there
  before K24: the projection and the pixel fetch in torch, the surviving rays materialised in
  chunks, ``OcTree.walk`` for their paths, then gathers, an exponential and a cumulative product in
  torch for the transmittance in front of the pair's own leaf, and an ``index_add_`` for the votes.
  Where a case has more pairs than ``--baseline-pairs`` the composition runs on every k-th leaf
  (all the case's cameras) and the comparison is per pair; the file says which;
* the experiment, at depth 8: carve from all but the last 4 cameras with ``color="mean"`` and with
  ``color="visible"``, hold those 4 out, every pixel of theirs against the ground-truth frame
  (colour, black background): the PSNR of both trees as built, of the visible tree as built at
  ``visible_transmittance`` 0.5, 0.3 and 0.1, and of both after ``fit_octree`` for 300 steps at the
  default learning rate, with the training loss at the first step, step 100 and the last.

    python scripts/microbench_octree_visible.py [--repeats 5] [--out result.json]
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
from scripts.microbench_octree_carve import (FIT_STEPS, HELD_OUT, psnr_all_pixels, quiet,  # noqa: E402
                                             torus_dataset)
from scripts.microbench_octree_render import device_ms  # noqa: E402

DEFAULT_OUT = os.path.join(ROOT, "profiles", "r22_octree_visible_microbench.json")
ALPHA_U8 = 128
TAU = 0.3
RAY_CHUNK = 1 << 17


def k24_inputs(tree, images_u8, cameras, center):
    dev = images_u8.device
    proj = torch.from_numpy(ffn.projection_matrices(cameras, origin=center)).to(dev)
    eyes = torch.from_numpy(ffn.eye_positions(cameras, center)).to(dev)
    return (tree._centers_on_device(), tree.scale, tree.depth, tree._on_device("node_index"),
            tree._on_device("leaf_index"), tree._colors_on_device(), 4, 3, images_u8, proj, eyes,
            ALPHA_U8, TAU)


def composed(tree, images_u8, proj, eyes, leaves, votes):
    """K24's answer for the leaves ``leaves`` (a device index tensor) from ops that were public
    before it -> (pairs that reached the walk).  ``votes`` (L,4) int64 is added to."""
    centers = tree._centers_on_device()[leaves]
    density = tree._colors_on_device()[:, 3].clamp_min(0.0).nan_to_num(0.0)
    height, width = images_u8.shape[1:3]
    cells = 1 << (tree.depth - 1)
    max_length = 3 * cells + 2                # room for every region of a chord
    walked = 0
    for c in range(proj.shape[0]):
        xyw = centers @ proj[c, :, :3].T + proj[c, :, 3]
        w = xyw[:, 2]
        fu, fv = xyw[:, 0] / w + 0.5, xyw[:, 1] / w + 0.5
        ok = (w > 0) & (fu >= 0) & (fu < width) & (fv >= 0) & (fv < height)
        col, row = fu.clamp(0, width - 1).long(), fv.clamp(0, height - 1).long()
        rgba = images_u8[c, torch.where(ok, row, 0), torch.where(ok, col, 0)]
        ok &= rgba[:, 3] >= ALPHA_U8
        which = torch.nonzero(ok)[:, 0]
        walked += int(which.numel())
        for begin in range(0, int(which.numel()), RAY_CHUNK):
            part = which[begin:begin + RAY_CHUNK]
            target = leaves[part]
            starts = eyes[c].expand(part.numel(), 3).contiguous()      # the rays, in memory
            directions = (centers[part] - starts).contiguous()
            path = tree.walk(starts, directions, max_length)
            t_in, hit = path.t_stops[:, :-1], path.leaves[:, :-1]
            t_out = path.t_stops[:, 1:]
            taken = (hit >= 0) & (t_out > 0)
            own = taken & (hit == target[:, None])
            chord = (t_out - t_in.clamp_min(0.0)) * directions.norm(dim=1, keepdim=True)
            sigma = density[hit.clamp_min(0)]
            keep = torch.where(taken & ~own, torch.exp(-(sigma * chord)), torch.ones_like(chord))
            through = torch.cumprod(keep, 1)
            before = torch.cat([torch.ones_like(through[:, :1]), through[:, :-1]], 1)
            seen = (own & (before > TAU)).any(1)
            add = torch.cat([rgba[part][seen][:, :3].long(),
                             torch.ones((int(seen.sum()), 1), dtype=torch.int64,
                                        device=seen.device)], 1)
            votes.index_add_(0, target[seen], add)
    return walked


def rejected_share(tree, images_u8, proj):
    """The share of all (leaf, camera) pairs that K24 rejects before the walk (torch f32)."""
    centers = tree._centers_on_device()
    height, width = images_u8.shape[1:3]
    passed = 0
    for c in range(proj.shape[0]):
        xyw = centers @ proj[c, :, :3].T + proj[c, :, 3]
        w = xyw[:, 2]
        fu, fv = xyw[:, 0] / w + 0.5, xyw[:, 1] / w + 0.5
        ok = (w > 0) & (fu >= 0) & (fu < width) & (fv >= 0) & (fv < height)
        col, row = fu.clamp(0, width - 1).long(), fv.clamp(0, height - 1).long()
        ok &= images_u8[c, torch.where(ok, row, 0), torch.where(ok, col, 0), 3] >= ALPHA_U8
        passed += int(ok.sum())
    return 1.0 - passed / (centers.shape[0] * proj.shape[0])


def kernel_case(tree, images_u8, cameras, center, repeats, baseline_pairs):
    args = k24_inputs(tree, images_u8, cameras, center)
    leaves, count = tree.num_leaves, len(cameras)
    pairs = leaves * count
    out = torch.zeros((leaves, 4), dtype=torch.uint32, device=images_u8.device)
    # the entry point alone: the op's checks read proj and eyes back, and it builds the blocks
    blocks = torch.cat([args[9].reshape(count, 12), args[10],
                        torch.zeros((count, 1), device=images_u8.device)], 1).contiguous()
    height, width = images_u8.shape[1:3]

    def launch():
        ops._call("ffn_octree_visible_votes", ops._dev(args[0]), ops.c_i64(leaves),
                  ops.c_f(tree.scale), ops.c_i(tree.depth), ops._dev(args[3], torch.int64),
                  ops.c_i64(args[3].numel()), ops._dev(args[4], torch.int64), ops._dev(args[5]),
                  ops.c_i(4), ops.c_i(3), ops._dev(images_u8, torch.uint8), ops._dev(blocks),
                  ops.c_i(count), ops.c_i(height), ops.c_i(width), ops.c_i(ALPHA_U8), ops.c_f(TAU),
                  ops._dev(out, torch.uint32))
    k24_ms = device_ms(launch, repeats)
    votes = ops.octree_visible_votes(*args).cpu().numpy().astype(np.int64)
    case = {"depth": tree.depth, "cameras": count, "leaves": leaves, "pairs": pairs,
            "k24_device_ms": k24_ms, "k24_leaves_per_s": leaves / (k24_ms * 1e-3),
            "k24_pairs_per_s": pairs / (k24_ms * 1e-3),
            "share_of_pairs_rejected_before_the_walk": rejected_share(tree, images_u8, args[9]),
            "share_of_pairs_visible": float(votes[:, 3].sum()) / pairs,
            "leaves_seen_by_no_camera": int((votes[:, 3] == 0).sum())}
    # the composition, on every k-th leaf where the case is too large for it
    stride = max(1, -(-pairs // baseline_pairs))
    sample = torch.arange(0, leaves, stride, device=images_u8.device)
    got = torch.zeros((leaves, 4), dtype=torch.int64, device=images_u8.device)
    walked = composed(tree, images_u8, args[9], args[10], sample, got)
    scratch = torch.zeros_like(got)
    base_ms = device_ms(lambda: composed(tree, images_u8, args[9], args[10], sample, scratch),
                        max(1, min(repeats, 2 if pairs > baseline_pairs else repeats)))
    sample_pairs = int(sample.numel()) * count
    same = got[sample].cpu().numpy() == votes[sample.cpu().numpy()]
    case.update({"composed_every_kth_leaf": stride, "composed_pairs": sample_pairs,
                 "composed_pairs_that_reached_the_walk": walked,
                 "composed_device_ms": base_ms,
                 "composed_pairs_per_s": sample_pairs / (base_ms * 1e-3),
                 "k24_speedup_per_pair": (base_ms / sample_pairs) / (k24_ms / pairs),
                 "composed_leaves_with_the_votes_of_k24": int(same.all(1).sum()),
                 "composed_leaves_compared": int(sample.numel())})
    return case


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--repeats", type=int, default=5)
    parser.add_argument("--depths", type=int, nargs="+", default=[8, 10])
    parser.add_argument("--camera-counts", type=int, nargs="+", default=[8, 120])
    parser.add_argument("--size", type=int, default=400)
    parser.add_argument("--truth-depth", type=int, default=9)
    parser.add_argument("--fit-depth", type=int, default=8)
    parser.add_argument("--baseline-pairs", type=int, default=1 << 22)
    parser.add_argument("--skip-experiment", action="store_true")
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
               "settings": "trees carved from all %d cameras with the defaults (cell_opacity 0.5, "
                           "no merging); alpha_u8 %d, min_transmittance %g; the composition walks "
                           "%d rays at a time" % (num_cameras, ALPHA_U8, TAU, RAY_CHUNK),
               "repeats": args.repeats, "rocprofv3_kernel_times": "not collected", "cases": []}
    dev = torch.device("cuda")
    whole = argparse.Namespace(images=images, cameras=cameras, color_space="RGB")
    for depth in args.depths:
        tree = ffn.OcTree.build_from_silhouettes(whole, depth, center, scale)
        for count in args.camera_counts:
            images_u8 = torch.from_numpy(np.ascontiguousarray(images[:count])).to(dev)
            case = kernel_case(tree, images_u8, cameras[:count], center, args.repeats,
                               args.baseline_pairs)
            results["cases"].append(case)
            print(json.dumps(case), flush=True)
            del images_u8
            torch.cuda.empty_cache()
        del tree
        torch.cuda.empty_cache()
    if not args.skip_experiment:
        results["experiment"] = experiment(images, cameras, bounds, center, scale, num_cameras,
                                           args.fit_depth)
    line = json.dumps(results, indent=1)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    return 0


def experiment(images, cameras, bounds, center, scale, num_cameras, depth):
    train_n = num_cameras - HELD_OUT
    train = quiet(ffn.ImageDataset, "train", images[:train_n], bounds, cameras[:train_n], 8,
                  device="cuda")
    held = quiet(ffn.ImageDataset, "val", images[train_n:], bounds, cameras[train_n:], 8,
                 device="cuda")

    def psnr(tree):
        return psnr_all_pixels(lambda starts, dirs: tree.render_volume(starts, dirs).color, held,
                               center)

    out = {"depth": depth, "train_cameras": train_n, "held_out_cameras": HELD_OUT,
           "fit_steps": FIT_STEPS}
    trees = {}
    for color in ("mean", "visible"):
        tree = ffn.OcTree.build_from_silhouettes(train, depth, center, scale, color=color)
        trees[color] = tree
        out["carved_leaves"] = tree.num_leaves
        out["psnr_as_built_" + color] = psnr(tree)
        print(color, "as built", out["psnr_as_built_" + color], flush=True)
    counts = trees["mean"].visible_votes(train, center)[:, 3]
    out["leaves_seen_by_no_camera"] = int((counts == 0).sum())
    out["mean_cameras_that_see_a_seen_leaf"] = float(counts[counts > 0].mean())
    for tau in (0.5, 0.3, 0.1):
        tree = ffn.OcTree.build_from_silhouettes(train, depth, center, scale, color="visible",
                                                 visible_transmittance=tau)
        out["psnr_as_built_visible_transmittance_%g" % tau] = psnr(tree)
        del tree
    for color in ("mean", "visible"):
        fitted, log = ffn.fit_octree(trees[color], train, None, num_steps=FIT_STEPS, verbose=False)
        out["psnr_after_fit_octree_" + color] = psnr(fitted)
        out["fit_loss_first_100_last_" + color] = [[e.step, e.loss]
                                                   for e in (log[0], log[min(100, len(log) - 1)],
                                                             log[-1])]
        print(color, "fitted", out["psnr_after_fit_octree_" + color], flush=True)
        del fitted
    return out


if __name__ == "__main__":
    sys.exit(main())
