"""Draws a triangle mesh (a Wavefront OBJ) from a dataset's cameras with the z-buffer rasteriser
(kernel K31): one PNG per camera and its PSNR against the camera's ground-truth image, in the
output format of ``scripts/render_octree.py``.  No counterpart in the reference.

An OBJ whose vertices read ``v x y z r g b`` (what ``scripts/octree_to_mesh.py`` writes) is drawn
with its vertex colours, any other with its texture (``--texture``, or the ``map_Kd`` of its
``mtllib``; white without one).  ``--normalize`` puts the mesh where
``scripts/make_mesh_npz.py`` put it when it made the dataset from the same file.

    python scripts/render_mesh.py mesh.obj data.npz out_dir [--normalize] [--supersample 4] [--antialias]
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
    ("--device", dict(default="cuda", help="Pytorch compute device")),
]


def build_parser():
    return _cli.build_parser("Mesh Renderer", RENDER_MESH)


def main():
    args = build_parser().parse_args()
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
    for camera in range(sampler.num_cameras):
        image = ffn.render_mesh_image(vertices, triangles, sampler.cameras[camera],
                                      background=args.background, supersample=args.supersample,
                                      device=device, antialias=args.antialias, **paint)
        _cli.save_png(os.path.join(args.output_dir, "frame_{:05d}.png".format(camera)), image)
        truth = ground_truth(dataset.images[camera], resolution, args.background)
        values.append(psnr(image, truth))
        print("camera %d (%s): psnr %.3f" % (camera, sampler.cameras[camera].name, values[-1]))
    print("mean psnr over %d cameras: %.3f" % (len(values), float(np.mean(values))))
    return 0


if __name__ == "__main__":
    sys.exit(main())
