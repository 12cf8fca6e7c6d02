"""Fits the leaf values of a baked octree (``scripts/bake_octree.py``, or a density tree of
``OcTree.build_from_model``) to the training images through the tree's own volume renderer
(``fit_octree``: kernels K15, K6, K17a-c, K7), and writes the fitted tree in the reference's file
format, ready for ``scripts/render_octree.py --mode volume``.  A tree whose file carries an
``sh_degree`` (``OcTree.bake_sh``) is fitted by ``fit_octree_sh`` (K18a, K6, K19a-c, K7) and keeps
its degree.  ``--tv-weight`` / ``--tv-eps`` switch the total-variation prior between touching
leaves on (K20), ``--dist-weight W`` the per-ray distortion prior (K29), which penalises rays that
spread their weight along a chord.  By default the structure of the tree does not change; ``--refine-rounds N`` makes
it ``fit_octree_adaptive`` (K21): N times fit, measure the per-leaf weights over the training rays,
drop the leaves below ``--prune-below`` and split those at or above ``--split-above``, then a last
fit; ``--steps`` is the length of every fit.  No counterpart in the reference.

The octree file has no place for the root cube's centre; ``voxelize_model.py`` prints it in the
form ``--center`` takes.

    python scripts/train_octree.py tree.npz data.npz out.npz --center X Y Z
"""

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scripts import _cli  # noqa: E402

# (flag, kwargs), as the tables of scripts/_cli.py
TRAIN_OCTREE = [
    ("tree_path", dict(help="Path to the baked octree NPZ")),
    ("data_path", dict(help="Path to the dataset NPZ")),
    ("output_path", dict(help="Path to the fitted octree NPZ")),
    ("--center", dict(type=float, nargs=3, default=[0.0, 0.0, 0.0], metavar=("X", "Y", "Z"),
                      help="Centre of the tree's root cube, as voxelize_model.py prints it")),
    ("--steps", dict(type=int, default=2000, help="Number of optimiser steps")),
    ("--lr", dict(type=float, default=None, help="Learning rate (default: fit_octree's)")),
    ("--batch-size", dict(type=int, default=4096, help="Rays per step")),
    ("--min-transmittance", dict(type=float, default=0.0,
                                 help="End a ray's walk once its transmittance is at or below this")),
    ("--report-interval", dict(type=int, default=500, help="Steps between validation reports")),
    ("--seed", dict(type=int, default=20080524, help="Seed of the ray shuffle")),
    ("--tv-weight", dict(type=float, nargs="+", default=None, metavar="W",
                         help="Weights of the total-variation prior (K20): RGB SIGMA for a plain "
                              "tree, BAND0 HIGHER_BANDS SIGMA for an SH tree (default: off)")),
    ("--tv-eps", dict(type=float, default=1e-2, help="The Charbonnier eps of the prior")),
    ("--dist-weight", dict(type=float, default=0.0, metavar="W",
                           help="Weight of the per-ray distortion prior (K29; default 0: off, "
                                "no tuned value)")),
    ("--refine-rounds", dict(type=int, default=0,
                             help="Rounds of fit -> measure -> prune / split before the last fit "
                                  "(K21; 0: the plain fit)")),
    ("--prune-below", dict(type=float, default=None,
                           help="Drop leaves whose largest ray weight is below this "
                                "(default: fit_octree_adaptive's, untuned)")),
    ("--split-above", dict(type=float, default=None,
                           help="Split leaves whose largest ray weight is at least this "
                                "(default: fit_octree_adaptive's, untuned)")),
    ("--max-depth", dict(type=int, default=None,
                         help="Deepest tree a split may make (default: the ray walk's limit)")),
    ("--device", dict(default="cuda", help="Pytorch compute device")),
]


def build_parser():
    return _cli.build_parser("Octree Trainer", TRAIN_OCTREE)


def main():
    args = build_parser().parse_args()
    device, _, _, _ = _cli.setup_device(args.device, False)
    import fourier_feature_nets_amd as ffn
    from fourier_feature_nets_amd import octree_fit
    tree = ffn.OcTree.load(args.tree_path)
    if tree is None:
        return 1
    train = ffn.ImageDataset.load(args.data_path, "train", 1, True, False, None, device=device)
    val = ffn.ImageDataset.load(args.data_path, "val", 1, True, False, None, device=device)
    if train is None or val is None:
        return 1
    lr = octree_fit.LEARNING_RATE if args.lr is None else args.lr
    fit = ffn.fit_octree
    if tree.sh_degree is not None:
        print("SH leaves of degree %d" % tree.sh_degree)
        fit = ffn.fit_octree_sh
    prior = {}
    if args.tv_weight is not None:
        want = 2 if tree.sh_degree is None else 3
        if len(args.tv_weight) != want:
            print("--tv-weight takes %d numbers for this tree (%s), got %d"
                  % (want, "RGB SIGMA" if want == 2 else "BAND0 HIGHER_BANDS SIGMA",
                     len(args.tv_weight)))
            return 1
        prior = dict(tv_weight=tuple(args.tv_weight), tv_eps=args.tv_eps)
        print("total-variation prior:", " ".join("%g" % w for w in args.tv_weight), "eps %g" % args.tv_eps)
    if args.dist_weight != 0.0:
        prior["dist_weight"] = args.dist_weight
        print("distortion prior: %g" % args.dist_weight)
    if args.refine_rounds > 0:
        policy = dict(max_depth=args.max_depth)
        if args.prune_below is not None:
            policy["prune_below"] = args.prune_below
        if args.split_above is not None:
            policy["split_above"] = args.split_above
        fitted, logs, _ = ffn.fit_octree_adaptive(
            tree, train, val, args.refine_rounds, batch_size=args.batch_size, learning_rate=lr,
            num_steps=args.steps, report_interval=args.report_interval, center=args.center,
            min_transmittance=args.min_transmittance, seed=args.seed, **policy, **prior)
        log = [entry for part in logs for entry in part]
    else:
        fitted, log = fit(tree, train, val, args.batch_size, lr, args.steps, args.report_interval,
                          center=args.center, min_transmittance=args.min_transmittance,
                          seed=args.seed, **prior)
    if log:
        print("loss first %.6g last %.6g over %d steps" % (log[0].loss, log[-1].loss, len(log)))
    fitted.save(args.output_path)
    print(fitted.num_leaves, "leaves fitted")
    return 0


if __name__ == "__main__":
    sys.exit(main())
