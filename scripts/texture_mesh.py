"""Fits a texture atlas for a triangle mesh (a Wavefront OBJ) to a dataset's images (kernel K33) and
writes the textured OBJ, its material library and the texture's PNG.  A mesh without a texture
(what ``scripts/octree_to_mesh.py`` and ``scripts/color_mesh.py`` write) is unwrapped first:
``unwrap_mesh`` gives every quad one ``--tile`` x ``--tile`` square of texels.  ``--init images``
starts every texel at the weighted mean of the pixels that see it (``texture_mesh_from_images``),
``--init colors`` at the OBJ's vertex colours (``bake_vertex_colors``; only for a mesh unwrapped
here), ``--init grey`` at 0.5, or at the OBJ's own texture when it has one; ``--fit STEPS`` then
optimises the texels against the images (``fit_mesh_texture``).  Prints the PSNR over the training
cameras and over the held-out split before and after.  No counterpart in the reference.

    python scripts/texture_mesh.py mesh.obj mesh_data.npz out.obj [--tile T]
        [--init images|colors|grey] [--fit STEPS]
"""

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scripts import _cli  # noqa: E402

# (flag, kwargs), as the tables of scripts/_cli.py
TEXTURE_MESH = [
    ("mesh_path", dict(help="Path to the OBJ file")),
    ("data_path", dict(help="Path to the dataset NPZ whose images texture the mesh")),
    ("output_path", dict(help="Path of the OBJ to write (its .mtl and .png land beside it)")),
    ("--tile", dict(type=int, default=4, help="texels a side of a quad's tile (>= 3)")),
    ("--init", dict(choices=["images", "colors", "grey"], default="images",
                    help="start from the cameras' mean colours, the OBJ's vertex colours or grey")),
    ("--fit", dict(type=int, default=0, metavar="STEPS", help="steps of fit_mesh_texture")),
    ("--split", dict(choices=["train", "val", "test"], default="train")),
    ("--held-out", dict(choices=["train", "val", "test"], default="val",
                        help="the split whose PSNR is reported beside the training split's")),
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
    return _cli.build_parser("Mesh Texturing", TEXTURE_MESH)


def mean_psnr(ffn, taps, texture, dataset):
    """The mean over the cameras of the PSNR of the K33b frame against the camera's pixels."""
    per = dataset.sampler.image_width * dataset.sampler.image_height
    values = []
    for number, camera_taps in enumerate(taps):
        color = ffn.render_mesh_texture(camera_taps, texture).color
        truth = dataset.colors[number * per:(number + 1) * per]
        error = float(((color - truth) ** 2).mean().item())
        values.append(-10.0 * np.log10(max(error, 1e-12)))
    return float(np.mean(values))


def split_size(path, split):
    """How many cameras ``split`` of the NPZ holds (found where ``ImageDataset.load`` finds it)."""
    if not os.path.exists(path):
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data",
                            path)
    data = np.load(path)
    train, val = (int(count) for count in data["split_counts"][:2])
    return dict(train=train, val=val, test=len(data["intrinsics"]) - train - val)[split]


def main():
    args = build_parser().parse_args()
    import torch
    import fourier_feature_nets_amd as ffn
    vertices, triangles, uvs, given, colors = ffn.load_obj(args.mesh_path, return_colors=True)
    textured = given.shape[:2] != (1, 1) or bool(np.any(uvs))
    if args.tile < 3 or args.fit < 0:
        print("texture_mesh: --tile must be >= 3 and --fit >= 0", file=sys.stderr)
        return 2
    if args.init == "colors" and (colors is None or textured):
        print("texture_mesh: --init colors needs an OBJ with vertex colours and without a "
              "texture", file=sys.stderr)
        return 2
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

    if textured:
        # the file's texture has row 0 at the top; the kernels' row index grows with v
        start = np.ascontiguousarray(given[::-1, :, :3]).astype(np.float32) / np.float32(255.0)
        size = start.shape[:2]
        print("%d vertices, %d triangles, the OBJ's own %d x %d texture"
              % (len(vertices), len(triangles), size[1], size[0]))
    else:
        flat_colors = colors
        vertices, triangles, uvs, vertex_map, size = ffn.unwrap_mesh(vertices, triangles, args.tile)
        start = np.full(size + (3,), 0.5, dtype=np.float32)
        if args.init == "colors":
            start = ffn.bake_vertex_colors(flat_colors[vertex_map], triangles, uvs, size, args.tile)
        print("%d vertices, %d triangles after unwrapping, a %d x %d atlas of %d x %d tiles"
              % (len(vertices), len(triangles), size[1], size[0], args.tile, args.tile))

    on = dict(device=device)
    v = torch.from_numpy(vertices).to(**on)
    t = torch.from_numpy(np.ascontiguousarray(triangles, dtype=np.int32)).to(**on)
    uv = torch.from_numpy(uvs).to(**on)
    texture = torch.from_numpy(start).to(**on)
    train_taps = [ffn.mesh_texture_taps(v, t, uv, camera, size)
                  for camera in dataset.sampler.cameras]
    held_taps = None if held_out is None else [ffn.mesh_texture_taps(v, t, uv, camera, size)
                                               for camera in held_out.sampler.cameras]

    def report(label, values):
        line = "%s: train psnr %.3f" % (label, mean_psnr(ffn, train_taps, values, dataset))
        if held_taps is not None:
            line += ", held-out psnr %.3f" % mean_psnr(ffn, held_taps, values, held_out)
        print(line)

    report("before", texture)
    if args.init == "images":
        texture, weights = ffn.texture_mesh_from_images(v, t, uv, dataset, size, texture,
                                                        args.alpha_threshold)
        print("init images: %d of %d texels seen" % (int((weights > 0).sum()), weights.numel()))
    if args.fit > 0:
        texture, log = ffn.fit_mesh_texture(v, t, uv, texture, dataset, None, num_steps=args.fit,
                                            learning_rate=args.learning_rate,
                                            cameras_per_step=args.cameras_per_step,
                                            seed=args.seed, verbose=False)
        print("fit: %d steps, loss %.6f -> %.6f" % (len(log), log[0].loss, log[-1].loss))
    report("after", texture)
    ffn.save_obj(args.output_path, vertices, triangles, uvs=uvs,
                 texture=ffn.texture_to_uint8(texture))
    print("wrote", args.output_path)
    return 0


if __name__ == "__main__":
    sys.exit(main())
