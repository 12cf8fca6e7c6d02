"""Trains a dense voxel radiance field on the MI355X path (counterpart of the reference's
train_voxels.py: same flags, same outputs `voxels.pt` + `log.txt`).  The checkpoint is what
`train_nerf.py`, `train_tiny_nerf.py` and `orbit_video.py` take as `--opacity-model`."""

import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fourier_feature_nets_amd as ffn  # noqa: E402
from scripts import _cli  # noqa: E402


def main():
    args = _cli.build_parser("Voxel Training Script", _cli.VOXELS).parse_args()
    args.device, _, _, _ = _cli.setup_device(args.device, False)
    torch.manual_seed(args.seed)
    include_alpha = args.mode == "rgba"
    train = ffn.ImageDataset.load(args.data_path, "train", args.num_samples, include_alpha, True,
                                  color_space=args.color_space, anneal_start=args.anneal_start,
                                  num_anneal_steps=args.num_anneal_steps, device=args.device)
    val = ffn.ImageDataset.load(args.data_path, "val", args.num_samples, include_alpha, False,
                                color_space=args.color_space, device=args.device)
    if train is None or val is None:
        return 1
    os.makedirs(args.results_dir, exist_ok=True)
    if args.make_video:        # same choice of visualizers as the reference driver
        hooks = [ffn.OrbitVideoVisualizer(args.results_dir, args.num_steps,
                                          train.cameras[0].resolution, args.num_frames,
                                          args.num_samples, args.color_space, device=args.device)]
    else:
        hooks = [ffn.EvaluationVisualizer(args.results_dir, ds, args.image_interval)
                 for ds in (train, val)]
    if args.mode == "dilate":
        train.mode = ffn.RayDataset.Mode.Dilate
    scale = 2 / float(train.sampler.bounds[0, 0])
    model = ffn.Voxels(args.side, scale)
    caster = ffn.Raycaster(model.to(args.device))
    log = caster.fit(train, val, args.batch_size, args.learning_rate, args.num_steps, 0,
                     args.report_interval, args.decay_rate, args.decay_steps, 0.0, hooks)
    model.save(os.path.join(args.results_dir, "voxels.pt"))
    _cli.write_log(os.path.join(args.results_dir, "log.txt"), args, log)
    # (train_voxels.py:123-124 of the reference also writes a scenepic HTML of the volume:
    # scenepic export is outside the HIP hot path -- SURVEY section 2)
    print("note: voxels.html (scenepic) is not written on the HIP path", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
