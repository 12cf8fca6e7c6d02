"""Carves an octree out of a dataset's silhouettes (kernel K23, ``OcTree.build_from_silhouettes``):
from the images (RGBA) and cameras of one split of a dataset NPZ to an ``.npz`` octree that
``scripts/train_octree.py`` fits and ``scripts/render_octree.py --mode volume`` renders, with no
trained model in between.  No counterpart in the reference.

    python scripts/carve_octree.py data.npz tree.npz [--split train] [--voxel-depth 8]
        [--center X Y Z] [--scale S] [--alpha-threshold 0.5] [--dilate 1] [--max-misses 0]
        [--min-views 2] [--cell-opacity 0.5] [--merge-tolerance RGB SIGMA]
        [--color {mean,visible}] [--visible-transmittance 0.3]
        [--footprint {point,box}] [--start-level 4]
        [--photo-threshold T] [--photo-min-views 2] [--photo-max-sweeps 16]

``--color visible`` colours every carved cell from the cameras that can see it through the carved
hull (kernel K24) instead of from all that look its way.  ``--footprint box`` carves conservatively
and coarse to fine from ``--start-level`` (kernel K27): a cell goes only when some camera sees its
whole projected footprint on the background, so thin structure survives and the hull is fatter.
``--photo-threshold T`` then thins the carved hull by photo-consistency (kernel K28a,
``OcTree.carve_photo``): sweep by sweep a cell goes when the cameras that see it disagree on its
colour by more than T (the root of the mean channel variance, colours in [0, 1]); the sweeps are
printed.  Off by default.
"""

import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scripts import _cli  # noqa: E402

# (flag, kwargs), as the tables of scripts/_cli.py
CARVE_OCTREE = [
    ("data_path", dict(help="Path to the dataset NPZ (images with alpha, cameras)")),
    ("output_path", dict(help="Path to the output octree")),
    ("--split", dict(choices=["train", "val", "test"], default="train")),
    ("--voxel-depth", dict(type=int, default=8, help="Depth of the octree to use")),
    ("--center", dict(type=float, nargs=3, default=[0.0, 0.0, 0.0], metavar=("X", "Y", "Z"),
                      help="Centre of the root cube")),
    ("--scale", dict(type=float, default=1.0, help="Half side of the root cube")),
    ("--alpha-threshold", dict(type=float, default=0.5,
                               help="A pixel is foreground at or above this alpha")),
    ("--dilate", dict(type=int, default=1, help="Pixels the silhouettes are grown by")),
    ("--max-misses", dict(type=int, default=0,
                          help="Cameras that may see a kept cell on the background")),
    ("--min-views", dict(type=int, default=2, help="Cameras that must see a kept cell")),
    ("--cell-opacity", dict(type=float, default=0.5,
                            help="Opacity of one cell side that the starting density gives")),
    ("--merge-tolerance", dict(type=float, nargs=2, default=None, metavar=("RGB", "SIGMA"),
                               help="Merge sibling cells that agree within these tolerances")),
    ("--batch-size", dict(type=int, default=1 << 20, help="Cells per kernel launch")),
    ("--color", dict(choices=["mean", "visible"], default="mean",
                     help="A cell's colour: the mean of every camera that looks at it, or of "
                          "those that see it through the carved hull")),
    ("--visible-transmittance", dict(type=float, default=0.3,
                                     help="--color visible: a camera sees a cell while the "
                                          "transmittance in front of it is above this")),
    ("--footprint", dict(choices=["point", "box"], default="point",
                         help="What a camera tests of a cell: its centre (K23), or the padded "
                              "rectangle round its centre and corners (K27, conservative)")),
    ("--start-level", dict(type=int, default=4,
                           help="--footprint box: the level the coarse-to-fine carve starts at")),
    ("--photo-threshold", dict(type=float, default=None, metavar="T",
                               help="Thin the hull by photo-consistency: drop a cell whose seeing "
                                    "cameras disagree on its colour by more than T (K28; off by "
                                    "default)")),
    ("--photo-min-views", dict(type=int, default=2,
                               help="--photo-threshold: cameras that must see a cell to judge it")),
    ("--photo-max-sweeps", dict(type=int, default=16,
                                help="--photo-threshold: sweeps at the most")),
    ("--device", dict(default="cuda", help="Pytorch compute device")),
]


def print_report(report):
    """One line per sweep of ``OcTree.carve_photo``."""
    for number, sweep in enumerate(report, 1):
        print("photo sweep %d: %d leaves, %d seen, %d judged, %d dropped"
              % (number, sweep.leaves, sweep.seen, sweep.judged, sweep.dropped))
    print("photo carve", "converged" if report.converged else "did not converge", "after",
          len(report), "sweeps")


def build_parser():
    return _cli.build_parser("Octree Carver", CARVE_OCTREE)


def main():
    args = build_parser().parse_args()
    device, _, _, _ = _cli.setup_device(args.device, False)
    import fourier_feature_nets_amd as ffn
    dataset = ffn.ImageDataset.load(args.data_path, args.split, 2, True, False, None,
                                    device=device)
    if dataset is None:
        return 1
    print("Carving", 8 ** (args.voxel_depth - 1), "cells with", dataset.num_cameras, "cameras")
    report = ffn.PhotoReport()
    tree = ffn.OcTree.build_from_silhouettes(
        dataset, args.voxel_depth, args.center, args.scale, args.alpha_threshold, args.dilate,
        args.max_misses, args.min_views, args.cell_opacity, args.merge_tolerance, args.batch_size,
        args.color, args.visible_transmittance, args.footprint, args.start_level,
        args.photo_threshold, args.photo_min_views, args.photo_max_sweeps, report)
    if args.photo_threshold is not None:
        print_report(report)
    print(tree.num_leaves, "leaves")
    # the file format is the reference's and has no place for the root cube's centre
    print("root cube centre (for train_octree.py / render_octree.py): --center",
          " ".join(np.format_float_positional(np.float32(c), trim="0") for c in tree.center))
    tree.save(args.output_path)
    return 0


if __name__ == "__main__":
    sys.exit(main())
