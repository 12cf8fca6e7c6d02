"""Thins an octree by photo-consistency (kernel K28a, ``OcTree.carve_photo``): sweep by sweep a leaf
goes when the cameras that can see it through the tree as it stands disagree on its colour, until a
sweep drops nothing.  What is left keeps its rows (``--recolor``: the mean of the cameras that see
it); the result is written in the reference's file format.  No counterpart in the reference.

The octree file has no place for the root cube's centre; ``carve_octree.py`` and
``voxelize_model.py`` print it in the form ``--center`` takes.

    python scripts/photo_carve_octree.py tree.npz data.npz out.npz --center X Y Z [--split train]
        [--threshold 0.1] [--min-views 2] [--max-sweeps 16] [--alpha-threshold 0.5]
        [--min-transmittance 0.3] [--recolor]
"""

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scripts import _cli  # noqa: E402
from scripts.carve_octree import print_report  # noqa: E402

# (flag, kwargs), as the tables of scripts/_cli.py
PHOTO_CARVE_OCTREE = [
    ("tree_path", dict(help="Path to the octree NPZ (leaves [r, g, b, sigma] or SH rows)")),
    ("data_path", dict(help="Path to the dataset NPZ (images with alpha, cameras)")),
    ("output_path", dict(help="Path to the thinned octree NPZ")),
    ("--center", dict(type=float, nargs=3, default=[0.0, 0.0, 0.0], metavar=("X", "Y", "Z"),
                      help="Centre of the tree's root cube, as carve_octree.py prints it")),
    ("--split", dict(choices=["train", "val", "test"], default="train",
                     help="The dataset split whose cameras judge")),
    ("--threshold", dict(type=float, default=0.1,
                         help="Drop a leaf whose seeing cameras disagree on its colour by more "
                              "than this (root of the mean channel variance, colours in [0, 1])")),
    ("--min-views", dict(type=int, default=2, help="Cameras that must see a leaf to judge it")),
    ("--max-sweeps", dict(type=int, default=16, help="Sweeps at the most")),
    ("--alpha-threshold", dict(type=float, default=0.5,
                               help="A pixel counts at or above this alpha")),
    ("--min-transmittance", dict(type=float, default=0.3,
                                 help="A camera sees a leaf while the transmittance in front of "
                                      "it is above this")),
    ("--recolor", dict(action="store_true",
                       help="Give every leaf that is left the mean of the cameras that see it")),
    ("--device", dict(default="cuda", help="Pytorch compute device")),
]


def build_parser():
    return _cli.build_parser("Octree Photo Carver", PHOTO_CARVE_OCTREE)


def main():
    args = build_parser().parse_args()
    device, _, _, _ = _cli.setup_device(args.device, False)
    import fourier_feature_nets_amd as ffn
    tree = ffn.OcTree.load(args.tree_path)
    if tree is None:
        return 1
    dataset = ffn.ImageDataset.load(args.data_path, args.split, 2, True, False, None,
                                    device=device)
    if dataset is None:
        return 1
    carved, report = tree.carve_photo(dataset, args.center, args.threshold, args.min_views,
                                      args.max_sweeps, args.alpha_threshold,
                                      args.min_transmittance, args.recolor)
    print_report(report)
    print(carved.num_leaves, "of", tree.num_leaves, "leaves left, judged by", dataset.num_cameras,
          "cameras")
    carved.save(args.output_path)
    return 0


if __name__ == "__main__":
    sys.exit(main())
