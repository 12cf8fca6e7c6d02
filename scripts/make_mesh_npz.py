"""Writes a dataset of a textured mesh in the reference's NPZ schema (images, intrinsics,
extrinsics, bounds, split_counts): a scene with real surfaces and smooth colour regions, with
ground-truth frames of any size, from nothing but the repository.  The mesh (an OBJ, or the
procedural torus) is sampled on the GPU (K22) and built into a colour octree; every camera of the
benchmark's synthetic rig is then rendered from the tree (first hit, flat shading), and a pixel's
alpha is 255 where its ray hit a leaf.  Schema, dtypes and split rule are those of
scripts/make_synthetic_npz.py.

``--render mesh`` draws the normalised mesh itself with the z-buffer rasteriser (K31) instead: the
frames show the surface and its texture, not the cells of a tree; a pixel's alpha is
``round(255 alpha)``, the covered share of its ``--supersample`` squared sub-pixels.  The tree is
then built only when ``--tree`` asks for it.  ``--render octree``, the default, writes the file it
always wrote.

    python scripts/make_mesh_npz.py out.npz [--mesh mesh.obj] [--voxel-depth 9] [--size 400]
        [--cameras 120] [--tree tree.npz] [--render {octree,mesh}] [--supersample 1]
"""

import argparse
import contextlib
import io
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("path")
    ap.add_argument("--mesh", help="OBJ file (default: the procedural torus)")
    ap.add_argument("--texture", help="image to use instead of the map_Kd of the OBJ's mtllib")
    ap.add_argument("--up-dir", default="0,1,0")
    ap.add_argument("--voxel-depth", type=int, default=9)
    ap.add_argument("--min-leaf-size", type=int, default=4)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--size", type=int, default=400)
    ap.add_argument("--cameras", type=int, default=120)
    ap.add_argument("--tree", help="also save the octree here")
    ap.add_argument("--render", choices=["octree", "mesh"], default="octree",
                    help="what the frames show: the mesh's colour octree, or the mesh itself")
    ap.add_argument("--supersample", type=int, default=1,
                    help="--render mesh: sub-pixels a side that every pixel averages")
    return ap


def parse_args(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.supersample < 1:
        ap.error("--supersample must be >= 1, got %d" % args.supersample)
    if args.supersample != 1 and args.render != "mesh":
        ap.error("--supersample belongs to --render mesh")
    return args


def main():
    args = parse_args()
    import fourier_feature_nets_amd as ffn
    from bench import synthetic_rig
    if args.mesh:
        mesh = ffn.load_obj(args.mesh, args.texture)
    else:
        mesh = ffn.procedural_torus()
    up_dir = [float(val) for val in args.up_dir.split(",")]
    tree = None
    if args.render == "octree" or args.tree:
        tree = ffn.OcTree.build_from_triangles(*mesh, args.voxel_depth, args.min_leaf_size, up_dir,
                                               args.seed)
        print(tree.num_leaves, "leaves; root cube centre (for render_octree.py): --center",
              " ".join(np.format_float_positional(np.float32(c), trim="0") for c in tree.center))
    if args.tree:
        tree.save(args.tree)
    intr, poses = synthetic_rig(args.cameras, args.size)
    cams = [ffn.CameraInfo.create("c%03d" % i, ffn.Resolution(args.size, args.size), intr, p)
            for i, p in enumerate(poses)]
    bounds = np.diag([2, 2, 2, 1]).astype(np.float32)
    images = np.zeros((args.cameras, args.size, args.size, 4), np.uint8)
    if args.render == "mesh":
        vertices, triangles, uvs, texture = mesh
        points = ffn.normalize_points(vertices, up_dir)
        for index in range(args.cameras):
            color, alpha, _ = ffn.render_mesh_image(points, triangles, cams[index], uvs=uvs,
                                                    texture=texture, include_depth=True,
                                                    supersample=args.supersample)
            images[index, ..., :3] = color
            images[index, ..., 3] = np.rint(255 * alpha)
    else:
        with contextlib.redirect_stdout(io.StringIO()):
            sampler = ffn.RaySampler(bounds, cams, 8)
        for index in range(args.cameras):
            color, alpha, _ = tree.render_image(sampler, index, shading="flat", include_depth=True)
            images[index, ..., :3] = color
            images[index, ..., 3] = np.where(alpha > 0, 255, 0)
    n_val = max(1, args.cameras // 17)
    n_test = max(1, args.cameras // 9)
    order = torch.randperm(args.cameras, generator=torch.Generator().manual_seed(0)).numpy()
    np.savez(args.path, images=images[order], intrinsics=np.stack([intr] * args.cameras),
             extrinsics=np.stack(poses)[order], bounds=bounds,
             split_counts=np.array([args.cameras - n_val - n_test, n_val, n_test], np.int32))
    print("wrote", args.path, images.shape, "hit share %.3f" % (images[..., 3] > 0).mean())


if __name__ == "__main__":
    main()
