"""Quality of the OPT-IN empty-space skipping during training (new semantics, DESIGN K9):
trains the tiny NeRF on the synthetic sphere scene three ways from the same weights and batches --
(A) the reference-exact step, (B) with the analytic occupancy grid from step 0, (C) the practical
recipe: full steps first, then a grid built from the model itself and refreshed periodically --
and reports validation PSNR (held-out cameras, full renders, vs the analytic images) and wall
time.   python scripts/skip_training_demo.py [--steps 1200] > profiles/r02_skip_training_demo.json
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench as B  # noqa: E402
import fourier_feature_nets_amd as ffn  # noqa: E402


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1200)
    ap.add_argument("--rays", type=int, default=16384)
    ap.add_argument("--cameras", type=int, default=48)
    ap.add_argument("--size", type=int, default=200)
    ap.add_argument("--warm", type=int, default=300, help="recipe C: full steps before the first grid")
    ap.add_argument("--refresh", type=int, default=300, help="recipe C: steps between grid rebuilds")
    return ap.parse_args(argv)


def make_scene(args, dev):
    """The protocol's scene (also scripts/skip_from_silhouettes_demo.py): the training dataset, the
    held-out sampler and frames, the valid ray ids and the analytic sphere grid."""
    intr, poses = B.synthetic_rig(args.cameras + 4, args.size)
    cams = [ffn.CameraInfo.create("c%03d" % i, ffn.Resolution(args.size, args.size), intr, p)
            for i, p in enumerate(poses)]
    bounds = np.diag([2, 2, 2, 1]).astype(np.float32)
    with contextlib.redirect_stdout(io.StringIO()):
        probe = ffn.RaySampler(bounds, cams, 64, device=dev)
        images = B.analytic_images(probe)
        del probe
        held = list(range(0, len(cams), len(cams) // 4))[:4]
        train_ids = [i for i in range(len(cams)) if i not in held]
        train = ffn.ImageDataset("train", images[train_ids], bounds, [cams[i] for i in train_ids], 64, True,
                                 True, anneal_start=0.2, num_anneal_steps=300, device=dev)
        val_sampler = ffn.RaySampler(bounds, [cams[i] for i in held], 64, device=dev)
    val_images = images[held][..., :3].astype(np.float32) / 255
    valid = train.sampler.valid.nonzero().reshape(-1)
    centres = ffn.OccupancyGrid.cell_centres(bounds, 128, dev)
    sphere = torch.zeros((centres.shape[0], 4), device=dev)
    sphere[:, 3] = torch.where(centres.norm(dim=1) < 0.6, 10.0, -30.0)
    analytic = ffn.OccupancyGrid.from_logits(sphere, bounds, 128, 0.01, True)
    del centres, sphere
    return argparse.Namespace(bounds=bounds, train=train, val_sampler=val_sampler, val_images=val_images,
                              valid=valid, held=held, train_ids=train_ids, analytic=analytic)


def psnr(scene, model, grid=None):
    caster = ffn.Raycaster(model)       # grid None = full render: every sample evaluated
    caster.occupancy = grid
    mse = 0.0
    for f in range(len(scene.held)):
        frame = caster.render_image(scene.val_sampler, f, 65536).astype(np.float32) / 255
        mse += float(np.mean((frame - scene.val_images[f]) ** 2))
    return -10 * np.log10(mse / len(scene.held))


def run_arm(scene, args, dev, grid=None, rebuild=None):
    """One training run of the protocol from the shared seeds.  ``grid``: imposed from step 0;
    ``rebuild(model, step)``: a grid to switch to before that step, or None."""
    torch.manual_seed(20080524)
    model = ffn.PositionalFourierMLP(3, 4, 5.5).to(dev)
    engine = ffn.TrainEngine(model, 0.0, None)
    gen = torch.Generator(device=dev).manual_seed(1)
    if grid is not None:
        engine.occupancy = grid
    fractions = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for step in range(args.steps):
        fresh = rebuild(model, step) if rebuild is not None else None
        if fresh is not None:
            engine.occupancy = fresh
        pick = torch.randint(0, scene.valid.numel(), (args.rays,), generator=gen, device=dev)
        lr = 5e-4 * 0.1 ** (step / 25000)
        engine.train_step(scene.train, scene.valid[pick], step, lr)
        if engine.occupancy is not None and step % 50 == 0:
            fractions.append(engine.last_evaluated_fraction)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    engine.check_finite()
    return {"val_psnr_db_full_render": round(psnr(scene, model), 3),
            "val_psnr_db_rendered_with_its_grid": (round(psnr(scene, model, engine.occupancy), 3)
                                                   if engine.occupancy is not None else None),
            "train_seconds": round(seconds, 2),
            "ms_per_step": round(1e3 * seconds / args.steps, 3),
            "mean_evaluated_sample_fraction": (round(float(np.mean(fractions)), 4)
                                               if fractions else 1.0)}


def scene_line(scene, args):
    return ("synthetic shaded sphere r=0.6, %d train / %d held-out cameras %dx%d, 64 samples/ray, "
            "%d rays/step, %d steps, tiny NeRF" % (len(scene.train_ids), len(scene.held), args.size,
                                                  args.size, args.rays, args.steps))


def main():
    args = parse_args()
    dev = torch.device("cuda:0")
    scene = make_scene(args, dev)

    def refreshed(model, step):
        if step >= args.warm and (step - args.warm) % args.refresh == 0:
            return ffn.OccupancyGrid.from_model(model, scene.bounds, 128, 0.01, True)
        return None

    results = {"A_full": run_arm(scene, args, dev),
               "B_analytic_grid": run_arm(scene, args, dev, grid=scene.analytic),
               "C_model_grid_refreshed": run_arm(scene, args, dev, rebuild=refreshed)}
    out = {"scene": scene_line(scene, args),
           "note": "A = reference-exact optimisation step; B, C = opt-in empty-space skipping during "
                   "training (samples in empty cells are sigma = 0 constants).  A grid that is imposed "
                   "from step 0 (B) leaves the density outside it untrained, so such a model must be "
                   "rendered with the same grid; a grid derived from the model after a full-step "
                   "warm-up (C) matches the exact run under the full render too", "runs": results}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
