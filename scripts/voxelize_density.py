"""Builds an octree with a leaf wherever a trained model has density
(``OcTree.build_from_model``, kernels K16): the model is evaluated at the centre of every cell of
the finest grid, and the leaves hold its own colour and density, so the file is ready for
``scripts/render_octree.py --mode volume`` without ``bake_octree.py``.  No counterpart in the
reference, whose ``voxelize_model.py`` makes the one-cell shell of the depth renders.

The octree file has no place for the root cube's centre; it is printed in the form
``render_octree.py --center`` takes.  A model that takes a view direction is evaluated for the one
fixed direction ``--view``.

    python scripts/voxelize_density.py model.pt tree.npz --voxel-depth 8
"""

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scripts import _cli  # noqa: E402

# (flag, kwargs), as the tables of scripts/_cli.py
VOXELIZE_DENSITY = [
    ("model_path", dict(help="Path to the saved model")),
    ("output_path", dict(help="Path to the octree NPZ")),
    ("--voxel-depth", dict(type=int, default=8,
                           help="Depth of the tree: the finest cells are 2^(depth-1) per axis")),
    ("--center", dict(type=float, nargs=3, default=[0.0, 0.0, 0.0], metavar=("X", "Y", "Z"),
                      help="Centre of the root cube")),
    ("--scale", dict(type=float, default=1.0, help="Half the side of the root cube")),
    ("--alpha-threshold", dict(type=float, default=0.01,
                               help="A cell is a leaf when its opacity along one side exceeds "
                                    "this")),
    ("--merge-tolerance", dict(type=float, nargs=2, default=None, metavar=("RGB", "SIGMA"),
                               help="Merge eight sibling leaves that lie within these of their "
                                    "mean")),
    ("--view", dict(type=float, nargs=3, default=[0.0, 0.0, 1.0], metavar=("X", "Y", "Z"),
                    help="The one view direction a view-dependent model is evaluated for")),
    ("--batch-size", dict(type=int, default=1 << 20,
                          help="Number of cells to evaluate in a batch")),
    ("--device", dict(default="cuda", help="Pytorch compute device")),
]


def build_parser():
    return _cli.build_parser("Density Voxelizer", VOXELIZE_DENSITY)


def main():
    args = build_parser().parse_args()
    device, _, _, _ = _cli.setup_device(args.device, False)
    import fourier_feature_nets_amd as ffn
    model = ffn.load_model(args.model_path)
    if model is None:
        return 1
    tree = ffn.OcTree.build_from_model(model.to(device), args.voxel_depth, args.center, args.scale,
                                       args.alpha_threshold, args.merge_tolerance, args.view,
                                       args.batch_size)
    print(tree.num_leaves, "leaves")
    # the file format is the reference's and has no place for the root cube's centre
    print("root cube centre (for render_octree.py): --center",
          " ".join(np.format_float_positional(np.float32(c), trim="0") for c in tree.center))
    tree.save(args.output_path)
    return 0


if __name__ == "__main__":
    sys.exit(main())
