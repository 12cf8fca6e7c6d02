"""One measure-and-refine of a baked or fitted octree, without fitting (K21): the per-leaf maximum
compositing weight over every ray of the dataset's training cameras (``leaf_weights_over``, K21a),
the threshold policy ``refine_actions``, and ``OcTree.refine`` (K21b), which drops the leaves no ray
sees with a weight worth keeping and splits the heavy ones into eight children that inherit their
values.  Prints the report and writes the refined tree in the reference's file format.  No
counterpart in the reference.

The octree file has no place for the root cube's centre; ``voxelize_model.py`` prints it in the
form ``--center`` takes.

    python scripts/refine_octree.py tree.npz data.npz out.npz --center X Y Z
"""

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scripts import _cli  # noqa: E402

# (flag, kwargs), as the tables of scripts/_cli.py
REFINE_OCTREE = [
    ("tree_path", dict(help="Path to the baked or fitted octree NPZ")),
    ("data_path", dict(help="Path to the dataset NPZ")),
    ("output_path", dict(help="Path to the refined octree NPZ")),
    ("--center", dict(type=float, nargs=3, default=[0.0, 0.0, 0.0], metavar=("X", "Y", "Z"),
                      help="Centre of the tree's root cube, as voxelize_model.py prints it")),
    ("--split", dict(default="train", help="The dataset split whose cameras measure the weights")),
    ("--prune-below", dict(type=float, default=None,
                           help="Drop leaves whose largest ray weight is below this "
                                "(default: fit_octree_adaptive's, untuned)")),
    ("--split-above", dict(type=float, default=None,
                           help="Split leaves whose largest ray weight is at least this "
                                "(default: fit_octree_adaptive's, untuned)")),
    ("--no-split", dict(action="store_true", help="Prune only")),
    ("--max-depth", dict(type=int, default=None,
                         help="Deepest tree a split may make (default: the ray walk's limit)")),
    ("--t-min", dict(type=float, default=0.0, help="Leaves that end before this t are not taken")),
    ("--min-transmittance", dict(type=float, default=0.0,
                                 help="End a ray's walk once its transmittance is at or below this")),
    ("--device", dict(default="cuda", help="Pytorch compute device")),
]


def build_parser():
    return _cli.build_parser("Octree Refiner", REFINE_OCTREE)


def main():
    args = build_parser().parse_args()
    device, _, _, _ = _cli.setup_device(args.device, False)
    import fourier_feature_nets_amd as ffn
    from fourier_feature_nets_amd import octree_fit
    tree = ffn.OcTree.load(args.tree_path)
    if tree is None:
        return 1
    data = ffn.ImageDataset.load(args.data_path, args.split, 1, True, False, None, device=device)
    if data is None:
        return 1
    prune_below = octree_fit.PRUNE_BELOW if args.prune_below is None else args.prune_below
    split_above = octree_fit.SPLIT_ABOVE if args.split_above is None else args.split_above
    if args.no_split:
        split_above = None
    weights = ffn.leaf_weights_over(tree, data, args.center, args.t_min, args.min_transmittance)
    report, refined = octree_fit.refine_once(tree, weights, 0, prune_below, split_above,
                                              args.max_depth)
    print(octree_fit.format_refine_report(report))
    refined.save(args.output_path)
    print(refined.num_leaves, "leaves written")
    return 0


if __name__ == "__main__":
    sys.exit(main())
