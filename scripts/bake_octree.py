"""Bakes a trained model into a voxelized octree (the ``.npz`` of ``scripts/voxelize_model.py``):
every leaf gets the model's own colour and density at its centre (``OcTree.bake``), so that
``scripts/render_octree.py --mode volume`` composites along the ray (kernel K15) where the
first-hit render shows one opaque colour per cell.  No counterpart in the reference.

The octree file has no place for the root cube's centre; ``voxelize_model.py`` prints it in the
form ``--center`` takes.  A model that takes a view direction is baked for the one fixed direction
``--view``: its view dependence is lost, unless ``--sh-degree`` is given.  Then every leaf gets
spherical-harmonic coefficients of the model's colour over ``--num-views`` view directions
(``OcTree.bake_sh``, kernel K18b); the file carries ``sh_degree`` and ``render_octree.py --mode
volume`` renders it per ray direction (kernel K18a) without a flag of its own.

    python scripts/bake_octree.py tree.npz model.pt out.npz --center X Y Z [--sh-degree 2]
"""

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scripts import _cli  # noqa: E402

# (flag, kwargs), as the tables of scripts/_cli.py
BAKE_OCTREE = [
    ("tree_path", dict(help="Path to the octree NPZ (voxelize_model.py's output)")),
    ("model_path", dict(help="Path to the saved model the tree was voxelized from")),
    ("output_path", dict(help="Path to the baked octree NPZ")),
    ("--center", dict(type=float, nargs=3, default=[0.0, 0.0, 0.0], metavar=("X", "Y", "Z"),
                      help="Centre of the tree's root cube, as voxelize_model.py prints it")),
    ("--view", dict(type=float, nargs=3, default=[0.0, 0.0, 1.0], metavar=("X", "Y", "Z"),
                    help="The one view direction a view-dependent model is baked for")),
    ("--batch-size", dict(type=int, default=1 << 20,
                          help="Number of leaves to evaluate in a batch")),
    ("--device", dict(default="cuda", help="Pytorch compute device")),
    ("--sh-degree", dict(type=int, choices=[1, 2], default=None,
                         help="Bake view-dependent colour as spherical harmonics of this degree")),
    ("--num-views", dict(type=int, default=64,
                         help="--sh-degree: number of view directions the model is sampled from")),
]


def build_parser():
    return _cli.build_parser("Octree Baker", BAKE_OCTREE)


def main():
    args = build_parser().parse_args()
    device, _, _, _ = _cli.setup_device(args.device, False)
    import fourier_feature_nets_amd as ffn
    tree = ffn.OcTree.load(args.tree_path)
    if tree is None:
        return 1
    model = ffn.load_model(args.model_path)
    if model is None:
        return 1
    if args.sh_degree is None:
        baked = tree.bake(model.to(device), center=args.center, view=args.view,
                          batch_size=args.batch_size)
        density = baked.leaf_data()[:, 3]
    else:
        baked = tree.bake_sh(model.to(device), args.sh_degree, args.num_views, center=args.center,
                             batch_size=args.batch_size)
        density = baked.leaf_data()[:, -1]
    print(baked.num_leaves, "leaves baked")
    print("density min %.6g median %.6g max %.6g" % (float(density.min()),
                                                      float(np.median(density)),
                                                      float(density.max())))
    baked.save(args.output_path)
    return 0


if __name__ == "__main__":
    sys.exit(main())
