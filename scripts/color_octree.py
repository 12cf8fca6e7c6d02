"""Recolours an octree from the cameras that can see each leaf (kernel K24,
``OcTree.color_from_images``): per leaf the mean of the pixels its centre projects to, over the
cameras whose ray to that centre is not blocked by the tree's own densities.  Leaves no camera sees
keep their colour.  Structure and densities are unchanged; the result is written in the reference's
file format.  No counterpart in the reference.

The octree file has no place for the root cube's centre; ``carve_octree.py`` and
``voxelize_model.py`` print it in the form ``--center`` takes.

    python scripts/color_octree.py tree.npz data.npz out.npz --center X Y Z [--split train]
        [--alpha-threshold 0.5] [--min-transmittance 0.3]
"""

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scripts import _cli  # noqa: E402

# (flag, kwargs), as the tables of scripts/_cli.py
COLOR_OCTREE = [
    ("tree_path", dict(help="Path to the octree NPZ (leaves [r, g, b, sigma])")),
    ("data_path", dict(help="Path to the dataset NPZ (images with alpha, cameras)")),
    ("output_path", dict(help="Path to the recoloured octree NPZ")),
    ("--center", dict(type=float, nargs=3, default=[0.0, 0.0, 0.0], metavar=("X", "Y", "Z"),
                      help="Centre of the tree's root cube, as carve_octree.py prints it")),
    ("--split", dict(choices=["train", "val", "test"], default="train",
                     help="The dataset split whose cameras vote")),
    ("--alpha-threshold", dict(type=float, default=0.5,
                               help="A pixel votes at or above this alpha")),
    ("--min-transmittance", dict(type=float, default=0.3,
                                 help="A camera sees a leaf while the transmittance in front of "
                                      "it is above this")),
    ("--device", dict(default="cuda", help="Pytorch compute device")),
]


def build_parser():
    return _cli.build_parser("Octree Colourer", COLOR_OCTREE)


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
    colored, counts = tree.color_from_images(dataset, args.center, args.alpha_threshold,
                                             args.min_transmittance)
    seen = int((counts > 0).sum())
    print(seen, "of", tree.num_leaves, "leaves recoloured from", dataset.num_cameras, "cameras;",
          tree.num_leaves - seen, "that no camera saw keep their colour")
    colored.save(args.output_path)
    return 0


if __name__ == "__main__":
    sys.exit(main())
