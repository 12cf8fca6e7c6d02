"""Draws a triangle mesh (a Wavefront OBJ) from a dataset's cameras with the z-buffer rasteriser
(kernel K31): one PNG per camera and its PSNR against the camera's ground-truth image, in the
output format of ``scripts/render_octree.py``.  No counterpart in the reference.

``--method rays`` casts the dataset sampler's own rays at the mesh instead (kernel K36, a tree over
the triangles and the first hit of every ray) and prints the same lines: it has no camera plane, so
it also draws what the rasteriser reports ``clipped``.  ``--supersample`` and ``--antialias`` are the
rasteriser's.

An OBJ whose vertices read ``v x y z r g b`` (what ``scripts/octree_to_mesh.py`` writes) is drawn
with its vertex colours, any other with its texture (``--texture``, or the ``map_Kd`` of its
``mtllib``; white without one).  ``--normalize`` puts the mesh where
``scripts/make_mesh_npz.py`` put it when it made the dataset from the same file.

    python scripts/render_mesh.py mesh.obj data.npz out_dir [--normalize] [--supersample 4] [--antialias]
    python scripts/render_mesh.py mesh.obj data.npz out_dir --method rays
"""

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scripts import _cli  # noqa: E402
from scripts.render_octree import ground_truth, psnr  # noqa: E402

# (flag, kwargs), as the tables of scripts/_cli.py
RENDER_MESH = [
    ("mesh_path", dict(help="Path to the OBJ file")),
    ("data_path", dict(help="Path to the dataset NPZ whose cameras are rendered")),
    ("output_dir", dict(help="Directory for the PNG frames")),
    ("--split", dict(choices=["train", "val", "test"], default="val")),
    ("--num-cameras", dict(type=int, default=10, help="Number of cameras to render")),
    ("--normalize", dict(action="store_true",
                         help="normalise the vertices as make_mesh_npz.py does (--up-dir)")),
    ("--up-dir", dict(default="0,1,0")),
    ("--texture", dict(help="image to use instead of the map_Kd of the OBJ's mtllib")),
    ("--background", dict(type=float, nargs=3, default=[0.0, 0.0, 0.0], metavar=("R", "G", "B"))),
    ("--supersample", dict(type=int, default=1,
                           help="sub-pixels a side that every pixel averages")),
    ("--antialias", dict(action="store_true",
                         help="blend the silhouette edges analytically (kernel K34a)")),
    ("--method", dict(choices=["raster", "rays"], default="raster",
                      help="the z-buffer rasteriser (K31), or a cast of the sampler's rays (K36)")),
    ("--device", dict(default="cuda", help="Pytorch compute device")),
]


def build_parser():
    return _cli.build_parser("Mesh Renderer", RENDER_MESH)


def cast_image(ffn, bvh, sampler, camera, paint, background):
    """The frame of ``camera`` from the sampler's own rays -> (H,W,3) uint8, K8's bytes."""
    import torch
    first = camera * sampler.rays_per_camera
    rays = slice(first, first + sampler.rays_per_camera)
    out = ffn.render_mesh_rays(bvh, sampler.starts[rays].contiguous(),
                               sampler.directions[rays].contiguous(), background=background, **paint)
    pixels = torch.arange(sampler.rays_per_camera, dtype=torch.int64, device=out.color.device)
    return ffn.ops.to_image(out.color.contiguous(), pixels, sampler.image_width,
                            sampler.image_height).cpu().numpy()


def main():
    args = build_parser().parse_args()
    if args.method == "rays" and (args.supersample != 1 or args.antialias):
        print("--supersample and --antialias belong to --method raster", file=sys.stderr)
        return 1
    device, _, _, _ = _cli.setup_device(args.device, False)
    import fourier_feature_nets_amd as ffn
    vertices, triangles, uvs, texture, colors = ffn.load_obj(args.mesh_path, args.texture,
                                                             return_colors=True)
    if args.normalize:
        vertices = ffn.normalize_points(vertices, [float(val) for val in args.up_dir.split(",")])
    paint = dict(colors=colors) if colors is not None else dict(uvs=uvs, texture=texture)
    dataset = ffn.ImageDataset.load(args.data_path, args.split, 2, True, False, None,
                                    device=device)
    if dataset is None:
        return 1
    if args.num_cameras < dataset.num_cameras:
        dataset = dataset.sample_cameras(args.num_cameras, 2, False)
    sampler = dataset.sampler
    os.makedirs(args.output_dir, exist_ok=True)
    resolution = (sampler.image_width, sampler.image_height)
    print("%d vertices, %d triangles, %s" % (len(vertices), len(triangles),
                                             "vertex colours" if colors is not None else "texture"))
    values = []
    bvh = ffn.build_mesh_bvh(vertices, triangles, device=device) if args.method == "rays" else None
    for camera in range(sampler.num_cameras):
        if bvh is not None:
            image = cast_image(ffn, bvh, sampler, camera, paint, args.background)
        else:
            image = ffn.render_mesh_image(vertices, triangles, sampler.cameras[camera],
                                          background=args.background,
                                          supersample=args.supersample, device=device,
                                          antialias=args.antialias, **paint)
        _cli.save_png(os.path.join(args.output_dir, "frame_{:05d}.png".format(camera)), image)
        truth = ground_truth(dataset.images[camera], resolution, args.background)
        values.append(psnr(image, truth))
        print("camera %d (%s): psnr %.3f" % (camera, sampler.cameras[camera].name, values[-1]))
    print("mean psnr over %d cameras: %.3f" % (len(values), float(np.mean(values))))
    return 0


if __name__ == "__main__":
    sys.exit(main())
