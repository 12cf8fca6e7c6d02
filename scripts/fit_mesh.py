"""Fits the vertex POSITIONS of a triangle mesh (a Wavefront OBJ) to a dataset's images through the
antialiased rasteriser (kernel K34, ``fit_mesh_geometry``).  The colours come from the images
(``color_mesh_from_images``, then ``--color-steps`` of ``fit_mesh_colors``), the geometry is fitted
with them held fixed, and the colours are taken again for the new geometry.  Prints, before and
after, the mean PSNR of ``render_mesh_image`` over the fitted cameras and over the held-out ones,
and the mean intersection over union of the drawn silhouette with the images' own alpha, and writes
the mesh with its new positions and colours.  No counterpart in the reference.

``--learning-rate``, ``--laplacian-weight`` and ``--max-displacement`` are untuned.  ``--interior``
adds the interior half of the geometry gradient (kernel K35: colour through the barycentric
weights); it is off by default.

    python scripts/fit_mesh.py mesh.obj data.npz out.obj [--steps N] [--learning-rate R]
        [--laplacian-weight W] [--max-displacement D] [--interior] [--color-steps N]
        [--split train]
"""

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scripts import _cli  # noqa: E402
from scripts.color_mesh import mean_psnr  # noqa: E402
from scripts.texture_mesh import split_size  # noqa: E402

# (flag, kwargs), as the tables of scripts/_cli.py
FIT_MESH = [
    ("mesh_path", dict(help="Path to the OBJ file")),
    ("data_path", dict(help="Path to the dataset NPZ whose images the mesh is fitted to")),
    ("output_path", dict(help="Path of the OBJ to write")),
    ("--steps", dict(type=int, default=300, help="steps of fit_mesh_geometry")),
    ("--learning-rate", dict(type=float, default=1e-3, help="untuned")),
    ("--laplacian-weight", dict(type=float, default=0.0,
                                help="weight of the displacement's smoothness term (untuned)")),
    ("--max-displacement", dict(type=float, default=None,
                                help="clamp on every component of the displacement (untuned)")),
    ("--interior", dict(action="store_true",
                        help="also move vertices by the colours sliding over their triangles "
                             "(K35); off by default")),
    ("--color-steps", dict(type=int, default=0,
                           help="steps of fit_mesh_colors after the colours are taken")),
    ("--split", dict(choices=["train", "val", "test"], default="train")),
    ("--held-out", dict(choices=["train", "val", "test"], default="val",
                        help="the split the held-out figures are measured on")),
    ("--cameras-per-step", dict(type=int, default=1)),
    ("--alpha-threshold", dict(type=float, default=0.5,
                               help="pixels whose alpha is below it colour nothing")),
    ("--normalize", dict(action="store_true",
                         help="normalise the vertices as make_mesh_npz.py does (--up-dir)")),
    ("--up-dir", dict(default="0,1,0")),
    ("--seed", dict(type=int, default=20080524)),
    ("--device", dict(default="cuda", help="Pytorch compute device")),
]


def build_parser():
    return _cli.build_parser("Mesh Geometry Fitting", FIT_MESH)


def silhouette_iou(ffn, vertices, triangles, colors, dataset, device):
    """The mean over the cameras of |drawn & truth| / |drawn | truth|: drawn where K31 puts a
    triangle, truth where the image's alpha byte is 128 or more.  NaN for images without alpha."""
    images = np.asarray(dataset.images)
    if images.shape[-1] != 4:
        return float("nan")
    values = []
    for number, camera in enumerate(dataset.sampler.cameras):
        _, ids, _ = ffn.render_mesh(vertices, triangles, camera, colors=colors, device=device,
                                    return_ids=True)
        drawn = ids >= 0
        truth = images[number][..., 3].reshape(-1) >= 128
        union = int((drawn | truth).sum())
        values.append(int((drawn & truth).sum()) / union if union else 1.0)
    return float(np.mean(values))


def main():
    args = build_parser().parse_args()
    import fourier_feature_nets_amd as ffn
    if args.steps < 0 or args.color_steps < 0:
        print("fit_mesh: --steps and --color-steps must be >= 0", file=sys.stderr)
        return 2
    vertices, triangles, _, _, _ = ffn.load_obj(args.mesh_path, return_colors=True)
    device, _, _, _ = _cli.setup_device(args.device, False)
    if args.normalize:
        vertices = ffn.normalize_points(vertices, [float(val) for val in args.up_dir.split(",")])
    dataset = ffn.ImageDataset.load(args.data_path, args.split, 2, True, False, None,
                                    device=device)
    if dataset is None:
        return 1
    held_out = None
    if args.held_out != args.split and split_size(args.data_path, args.held_out) > 0:
        held_out = ffn.ImageDataset.load(args.data_path, args.held_out, 2, True, False, None,
                                         device=device)
    print("%d vertices, %d triangles, %d cameras, %d held out" % (
        len(vertices), len(triangles), dataset.num_cameras,
        0 if held_out is None else held_out.num_cameras))

    def colour(positions):
        colors, _ = ffn.color_mesh_from_images(positions, triangles, dataset, None,
                                               args.alpha_threshold)
        if args.color_steps > 0:
            colors, _ = ffn.fit_mesh_colors(positions, triangles, colors, dataset, None,
                                            num_steps=args.color_steps,
                                            cameras_per_step=args.cameras_per_step,
                                            seed=args.seed, verbose=False)
        return colors

    def report(label, positions, colors):
        line = "%s: mean psnr %.3f" % (label, mean_psnr(ffn, positions, triangles, colors, dataset,
                                                        device))
        measured = dataset
        if held_out is not None:
            measured = held_out
            line += ", held-out psnr %.3f" % mean_psnr(ffn, positions, triangles, colors, held_out,
                                                       device)
        print(line + ", silhouette iou %.4f" % silhouette_iou(ffn, positions, triangles, colors,
                                                              measured, device))

    colors = colour(vertices)
    report("before", vertices, colors)
    fitted = vertices
    if args.steps > 0:
        fitted, log = ffn.fit_mesh_geometry(
            vertices, triangles, colors, dataset, None, num_steps=args.steps,
            learning_rate=args.learning_rate, cameras_per_step=args.cameras_per_step,
            laplacian_weight=args.laplacian_weight, max_displacement=args.max_displacement,
            seed=args.seed, verbose=False, interior=args.interior)
        moved = np.linalg.norm(fitted - vertices, axis=1)
        print("fit: %d steps, loss %.6f -> %.6f, mean displacement %.5f, largest %.5f"
              % (len(log), log[0].loss, log[-1].loss, moved.mean(), moved.max()))
        colors = colour(fitted)
    report("after", fitted, colors)
    ffn.save_obj(args.output_path, fitted, triangles, colors)
    print("wrote", args.output_path)
    return 0


if __name__ == "__main__":
    sys.exit(main())
