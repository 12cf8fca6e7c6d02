"""Voxelizes a trained model into a sparse octree on the MI355X path (counterpart of the
reference's voxelize_model.py: same arguments, same ``.npz`` output): renders depth maps of the
training cameras, turns every opaque ray into a surface point (kernel K12a-d) and builds the
octree from the cloud (K12e-i).  The cloud never leaves the GPU."""

import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fourier_feature_nets_amd as ffn  # noqa: E402
from fourier_feature_nets_amd import ops  # noqa: E402
from scripts import _cli  # noqa: E402


def main():
    args = _cli.build_parser("Model Voxelizer", _cli.VOXELIZE).parse_args()
    device, _, _, _ = _cli.setup_device(args.device, False)
    model = ffn.load_model(args.model_path)
    if model is None:
        return 1
    opacity_model = None
    if args.opacity_model_path:
        opacity_model = ffn.load_model(args.opacity_model_path).to(device)
    # (positionally 400 samples per ray and a truthy include_alpha, as voxelize_model.py:48-49)
    dataset = ffn.ImageDataset.load(args.data_path, "train", 400, 128, False, opacity_model,
                                    device=device)
    if dataset is None:
        return 1
    if args.num_cameras < dataset.num_cameras:
        dataset = dataset.sample_cameras(args.num_cameras, dataset.num_samples, False)
    sampler = dataset.sampler
    raycaster = ffn.Raycaster(model.to(device))
    num_rays = len(sampler)
    positions, colors = [], []
    bar = ffn.ETABar("Sampling the model", max=num_rays)
    with torch.no_grad():
        for start in range(0, num_rays, args.batch_size):
            end = min(start + args.batch_size, num_rays)
            index = torch.arange(start, end, dtype=torch.int64, device=sampler.device)
            color, alpha, depth = raycaster.render(sampler.sample(index, None), True)
            position, kept, count = ops.octree_surface_points(
                alpha.contiguous(), depth.contiguous(), sampler.starts[index].contiguous(),
                sampler.directions[index].contiguous(), args.alpha_threshold, color.contiguous())
            count = int(count.item())       # the one read-back of the batch
            positions.append(position[:count])
            colors.append(kept[:count])
            bar.next(end - start)
    bar.finish()
    raycaster.check_finite()
    positions = torch.cat(positions)
    colors = torch.cat(colors)
    print(len(positions), "points in cloud")
    voxels = ffn.OcTree.build_from_samples(positions, args.voxel_depth, args.min_leaf_size, colors)
    # the file format is the reference's and has no place for the root cube's centre
    print("root cube centre (for render_octree.py): --center",
          " ".join(np.format_float_positional(np.float32(c), trim="0") for c in voxels.center))
    voxels.save(args.output_path)
    if args.scenepic_path:
        # (voxelize_model.py:90-110 of the reference writes a scenepic HTML of the leaf cubes)
        print("warning: --scenepic-path is not supported on the HIP path (scenepic is not "
              "available); no HTML is written", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
