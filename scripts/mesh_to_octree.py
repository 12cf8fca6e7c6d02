"""Turns a textured OBJ mesh into a colour octree on the MI355X path (counterpart of the
reference's figures/mesh_to_octree.py: same arguments and defaults, same ``.npz`` output): the
surface samples are drawn on the GPU (kernel K22) and the octree is built from the cloud where it
lies (K12e-i).

    python scripts/mesh_to_octree.py mesh.obj out.npz [--voxel-depth 8] [--min-leaf-size 4]
        [--up-dir 0,1,0] [--texture file] [--seed 0]
"""

import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fourier_feature_nets_amd as ffn  # noqa: E402


def main():
    parser = argparse.ArgumentParser("Mesh Voxelizer")
    parser.add_argument("mesh_path", help="Path to the OBJ file")
    parser.add_argument("output_path", help="Path to the output NPZ")
    parser.add_argument("--voxel-depth", type=int, default=8, help="Depth of the octree to use")
    parser.add_argument("--min-leaf-size", type=int, default=4,
                        help="Minimum number of samples in a leaf")
    parser.add_argument("--up-dir", default="0,1,0")
    parser.add_argument("--texture", help="Image to use instead of the map_Kd of the mtllib")
    parser.add_argument("--seed", type=int, default=0,
                        help="Seed of the per-triangle sample counts")
    args = parser.parse_args()
    up_dir = [float(val) for val in args.up_dir.split(",")]

    print("Loading model...")
    vertices, triangles, uvs, texture = ffn.load_obj(args.mesh_path, args.texture)
    print(len(vertices), "vertices,", len(triangles), "triangles, texture", texture.shape)
    print("Sampling", (8 ** (args.voxel_depth - 2)) * args.min_leaf_size,
          "positions on the surface of the mesh and building the octree")
    voxels = ffn.OcTree.build_from_triangles(vertices, triangles, uvs, texture, args.voxel_depth,
                                             args.min_leaf_size, up_dir, args.seed)
    print(voxels.num_leaves, "leaves")
    # the file format is the reference's and has no place for the root cube's centre
    print("root cube centre (for render_octree.py): --center",
          " ".join(np.format_float_positional(np.float32(c), trim="0") for c in voxels.center))
    voxels.save(args.output_path)
    return 0


if __name__ == "__main__":
    sys.exit(main())
