"""Renders a voxelized model (the ``.npz`` octree of ``scripts/voxelize_model.py``) from a
dataset's cameras with the first-hit walk (kernel K14): one PNG per camera and its PSNR against
the camera's ground-truth image.  No counterpart in the reference, which shows the leaf cubes
through scenepic (voxelize_model.py:90-110).  ``--mode volume`` composites a tree that
``scripts/bake_octree.py`` has baked along the whole ray instead (kernel K15); a file baked with
``--sh-degree`` says so itself and gets its view-dependent colour (kernel K18a).

The octree file has no place for the root cube's centre; ``voxelize_model.py`` prints it in the
form ``--center`` takes.

    python scripts/render_octree.py tree.npz data.npz out_dir --center X Y Z
"""

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scripts import _cli  # noqa: E402

# (flag, kwargs), as the tables of scripts/_cli.py
RENDER_OCTREE = [
    ("tree_path", dict(help="Path to the octree NPZ (voxelize_model.py's output)")),
    ("data_path", dict(help="Path to the dataset NPZ whose cameras are rendered")),
    ("output_dir", dict(help="Directory for the PNG frames")),
    ("--split", dict(choices=["train", "val", "test"], default="val")),
    ("--resolution", dict(type=int, default=None,
                          help="Frame height in pixels (default: the dataset's own)")),
    ("--num-cameras", dict(type=int, default=10, help="Number of cameras to render")),
    ("--center", dict(type=float, nargs=3, default=[0.0, 0.0, 0.0], metavar=("X", "Y", "Z"),
                      help="Centre of the tree's root cube, as voxelize_model.py prints it")),
    ("--shading", dict(choices=["flat", "faces"], default="flat")),
    ("--background", dict(type=float, nargs=3, default=[0.0, 0.0, 0.0], metavar=("R", "G", "B"))),
    ("--device", dict(default="cuda", help="Pytorch compute device")),
    ("--mode", dict(choices=["first-hit", "volume"], default="first-hit",
                    help="first-hit: one opaque colour per cell; volume: composite a baked tree")),
    ("--min-transmittance", dict(type=float, default=0.0,
                                 help="volume: a ray ends once its transmittance is at or below")),
]


def build_parser():
    return _cli.build_parser("Octree Renderer", RENDER_OCTREE)


def ground_truth(image, resolution, background):
    """(H,W,3|4) u8 -> (h,w,3) u8 at the frame's size: the dataset's colours, the background
    where alpha is 0 (the dataset zeroes them, image_dataset.py:244-262)."""
    if (image.shape[1], image.shape[0]) != tuple(resolution):
        from PIL import Image
        image = np.asarray(Image.fromarray(image).resize(tuple(resolution), Image.BILINEAR))
    rgb = image[..., :3]
    if image.shape[-1] == 4:
        fill = np.clip(np.round(np.asarray(background) * 255), 0, 255).astype(np.uint8)
        rgb = np.where(image[..., 3:] > 0, rgb, fill[None, None, :])
    return rgb


def psnr(a, b):
    err = ((a.astype(np.float64) - b.astype(np.float64)) / 255.0) ** 2
    return float(-10 * np.log10(max(err.mean(), 1e-12)))


def main():
    args = build_parser().parse_args()
    device, _, _, _ = _cli.setup_device(args.device, False)
    import fourier_feature_nets_amd as ffn
    from fourier_feature_nets_amd.cameras import CameraInfo
    tree = ffn.OcTree.load(args.tree_path)
    if tree is None:
        return 1
    dataset = ffn.ImageDataset.load(args.data_path, args.split, 2, True, False, None,
                                    device=device)
    if dataset is None:
        return 1
    if args.num_cameras < dataset.num_cameras:
        dataset = dataset.sample_cameras(args.num_cameras, 2, False)
    sampler = dataset.sampler
    if args.resolution and args.resolution != dataset.image_height:
        cameras = []
        for cam in sampler.cameras:
            res = cam.resolution.scale_to_height(args.resolution)
            k = np.array(cam.intrinsics, np.float32)
            k[0] *= res.width / cam.resolution.width
            k[1] *= res.height / cam.resolution.height
            cameras.append(CameraInfo.create(cam.name, res, k, cam.extrinsics))
        sampler = ffn.RaySampler(sampler.bounds, cameras, 2, device=device)
    os.makedirs(args.output_dir, exist_ok=True)
    resolution = (sampler.image_width, sampler.image_height)
    values = []
    for camera in range(sampler.num_cameras):
        image = tree.render_image(sampler, camera, center=args.center,
                                  background=args.background, shading=args.shading,
                                  mode=args.mode.replace("-", "_"),
                                  min_transmittance=args.min_transmittance)
        _cli.save_png(os.path.join(args.output_dir, "frame_{:05d}.png".format(camera)), image)
        truth = ground_truth(dataset.images[camera], resolution, args.background)
        values.append(psnr(image, truth))
        print("camera %d (%s): psnr %.3f" % (camera, sampler.cameras[camera].name, values[-1]))
    print("mean psnr over %d cameras: %.3f" % (len(values), float(np.mean(values))))
    return 0


if __name__ == "__main__":
    sys.exit(main())
