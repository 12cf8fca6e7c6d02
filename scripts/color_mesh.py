"""Colours the vertices of a triangle mesh (a Wavefront OBJ) from a dataset's images (kernel K32):
``--init images`` gives every vertex the mean colour of the pixels that see it
(``color_mesh_from_images``), ``--fit STEPS`` then optimises the colours against the images through
the rasteriser (``fit_mesh_colors``).  Prints the mean PSNR of ``render_mesh_image`` over the
cameras before and after and writes the mesh with its new colours (``v x y z r g b``).  No
counterpart in the reference.

``--init given`` starts from the colours of the OBJ (what ``scripts/octree_to_mesh.py`` writes); a
mesh without colours needs ``--init images``.  ``--normalize`` as in ``scripts/render_mesh.py``.

    python scripts/color_mesh.py mesh.obj data.npz out.obj [--init images|given] [--fit STEPS]
"""

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scripts import _cli  # noqa: E402
from scripts.render_octree import ground_truth, psnr  # noqa: E402

# (flag, kwargs), as the tables of scripts/_cli.py
COLOR_MESH = [
    ("mesh_path", dict(help="Path to the OBJ file")),
    ("data_path", dict(help="Path to the dataset NPZ whose images colour the mesh")),
    ("output_path", dict(help="Path of the OBJ to write")),
    ("--init", dict(choices=["images", "given"], default="images",
                    help="start from the cameras' mean colours, or from the OBJ's own")),
    ("--fit", dict(type=int, default=0, metavar="STEPS", help="steps of fit_mesh_colors")),
    ("--split", dict(choices=["train", "val", "test"], default="train")),
    ("--learning-rate", dict(type=float, default=1e-2, help="untuned")),
    ("--cameras-per-step", dict(type=int, default=1)),
    ("--alpha-threshold", dict(type=float, default=0.5,
                               help="pixels whose alpha is below it colour nothing (--init images)")),
    ("--normalize", dict(action="store_true",
                         help="normalise the vertices as make_mesh_npz.py does (--up-dir)")),
    ("--up-dir", dict(default="0,1,0")),
    ("--seed", dict(type=int, default=20080524)),
    ("--device", dict(default="cuda", help="Pytorch compute device")),
]


def build_parser():
    return _cli.build_parser("Mesh Colouring", COLOR_MESH)


def mean_psnr(ffn, vertices, triangles, colors, dataset, device):
    sampler = dataset.sampler
    resolution = (sampler.image_width, sampler.image_height)
    values = []
    for camera in range(sampler.num_cameras):
        image = ffn.render_mesh_image(vertices, triangles, sampler.cameras[camera], colors=colors,
                                      device=device)
        values.append(psnr(image, ground_truth(dataset.images[camera], resolution, (0, 0, 0))))
    return float(np.mean(values))


def main():
    args = build_parser().parse_args()
    import fourier_feature_nets_amd as ffn
    vertices, triangles, _, _, colors = ffn.load_obj(args.mesh_path, return_colors=True)
    if colors is None and args.init != "images":
        print("color_mesh: %s has no vertex colours; --init given needs them (--init images "
              "takes them from the cameras)" % args.mesh_path, file=sys.stderr)
        return 2
    if args.fit < 0:
        print("color_mesh: --fit must be >= 0", file=sys.stderr)
        return 2
    device, _, _, _ = _cli.setup_device(args.device, False)
    if args.normalize:
        vertices = ffn.normalize_points(vertices, [float(val) for val in args.up_dir.split(",")])
    dataset = ffn.ImageDataset.load(args.data_path, args.split, 2, True, False, None,
                                    device=device)
    if dataset is None:
        return 1
    start = np.full(vertices.shape, 0.5, dtype=np.float32) if colors is None else colors
    print("%d vertices, %d triangles, %d cameras, %s" % (
        len(vertices), len(triangles), dataset.num_cameras,
        "vertex colours" if colors is not None else "no colours (0.5 grey)"))
    print("before: mean psnr %.3f" % mean_psnr(ffn, vertices, triangles, start, dataset, device))
    colors = start
    if args.init == "images":
        colors, weights = ffn.color_mesh_from_images(vertices, triangles, dataset, start,
                                                     args.alpha_threshold)
        print("init images: %d of %d vertices seen, mean psnr %.3f" % (
            int((weights > 0).sum()), len(vertices),
            mean_psnr(ffn, vertices, triangles, colors, dataset, device)))
    if args.fit > 0:
        colors, log = ffn.fit_mesh_colors(vertices, triangles, colors, dataset, None,
                                          num_steps=args.fit, learning_rate=args.learning_rate,
                                          cameras_per_step=args.cameras_per_step, seed=args.seed,
                                          verbose=False)
        print("fit: %d steps, loss %.6f -> %.6f" % (len(log), log[0].loss, log[-1].loss))
    print("after: mean psnr %.3f" % mean_psnr(ffn, vertices, triangles, colors, dataset, device))
    ffn.save_obj(args.output_path, vertices, triangles, colors)
    print("wrote", args.output_path)
    return 0


if __name__ == "__main__":
    sys.exit(main())
