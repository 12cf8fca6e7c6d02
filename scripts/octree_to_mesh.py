"""Turns an octree ``.npz`` (this project's or the reference's) into a coloured triangle mesh that any
viewer, slicer or DCC tool opens: ``OcTree.extract_mesh`` on the GPU (kernel K30), then a Wavefront
OBJ with per-vertex colours and normals.

    python scripts/octree_to_mesh.py tree.npz out.obj [--alpha-threshold 0.5]
        [--placement surface_nets|corners] [--center X Y Z]
"""

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fourier_feature_nets_amd as ffn  # noqa: E402


def main():
    parser = argparse.ArgumentParser("Octree Mesher")
    parser.add_argument("octree_path", help="Path to the octree NPZ")
    parser.add_argument("output_path", help="Path to the output OBJ")
    parser.add_argument("--alpha-threshold", type=float, default=0.5,
                        help="A finest cell is solid when its opacity exceeds this")
    parser.add_argument("--placement", choices=("surface_nets", "corners"),
                        default="surface_nets",
                        help="Smooth vertex placement, or the exact block surface")
    parser.add_argument("--center", type=float, nargs=3, metavar=("X", "Y", "Z"),
                        help="Centre of the root cube (the file does not hold it); default 0 0 0")
    args = parser.parse_args()

    tree = ffn.OcTree.load(args.octree_path)
    if tree is None:
        return 1
    print(tree.num_leaves, "leaves, depth", tree.depth)
    mesh = tree.extract_mesh(args.alpha_threshold, args.placement, args.center)
    print(len(mesh.vertices), "vertices,", len(mesh.triangles), "triangles")
    ffn.save_obj(args.output_path, mesh.vertices, mesh.triangles, mesh.colors, mesh.normals)
    return 0


if __name__ == "__main__":
    sys.exit(main())
