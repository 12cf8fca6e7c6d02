"""Shared pieces of the driver scripts: table-driven argument parsers with the reference
drivers' flag names and defaults, log writing, and a small PNG-dumping training hook."""

import argparse
import json
import os

import numpy as np

# not a flag of the reference: how --opacity-model drives the focus samples.  "table" = the
# reference's per-ray CDF table built at start-up (ray_sampler.py:148-166); "live" = no table, the
# coarse model is evaluated per batch inside the sampling kernel -- bit-identical t-values for a
# frozen opacity model, which a checkpoint loaded by these drivers always is, so "auto" means live
FOCUS_MODE = ("--focus-mode", dict(choices=["auto", "table", "live"], default="auto"))

# (flag, kwargs) -- names/defaults follow train_nerf.py:14-71, train_tiny_nerf.py:14-66 and
# orbit_video.py:16-40 of the reference so that command lines carry over unchanged
TRAIN_COMMON = [
    ("data_path", dict(help="dataset NPZ")),
    ("results_dir", dict(help="output directory")),
    ("--mode", dict(choices=["rgba", "rgb", "dilate"], default="rgba")),
    ("--opacity-model", dict(help="checkpoint of a coarse opacity model (focus sampling)")),
    ("--num-samples", dict(type=int, default=128)),
    ("--batch-size", dict(type=int, default=1024)),
    ("--learning-rate", dict(type=float, default=5e-4)),
    ("--num-channels", dict(type=int, default=256)),
    ("--num-steps", dict(type=int, default=50000)),
    ("--report-interval", dict(type=int, default=1000)),
    ("--image-interval", dict(type=int, default=2000)),
    ("--crop-steps", dict(type=int, default=1000)),
    ("--seed", dict(type=int, default=20080524)),
    ("--decay-rate", dict(type=float, default=0.1)),
    ("--weight-decay", dict(type=float, default=0)),
    ("--make-video", dict(action="store_true")),
    ("--color-space", dict(choices=["YCrCb", "RGB"], default="RGB")),
    ("--num-frames", dict(type=int, default=200)),
    ("--device", dict(default="cuda")),
    ("--anneal-start", dict(type=float, default=0.2)),
    ("--num-anneal-steps", dict(type=int, default=2000)),
    # not a flag of the reference: the opt-in split-bf16 kernels, training and renders
    ("--precision", dict(choices=["f32", "bf16x3", "bf16x6"], default="f32")),
    # not flags of the reference either: opt-in empty-space skipping during training (DESIGN K9):
    # exact steps for --skip-warmup steps, then an occupancy grid derived from the model and
    # rebuilt every --skip-refresh steps
    ("--skip-empty-space", dict(action="store_true")),
    ("--skip-warmup", dict(type=int, default=1000)),
    ("--skip-refresh", dict(type=int, default=500)),
    FOCUS_MODE,
]
# not flags of the reference either: a grid that needs no model, imposed from step 0 (DESIGN K25),
# from a saved octree or carved from the training images' silhouettes at this depth (0 = off).  A
# table of its own, appended by the two NeRF drivers: TRAIN_COMMON stays what it was
SKIP_GRID = [
    ("--skip-tree", dict(help="octree NPZ whose leaves become the occupancy grid")),
    ("--skip-tree-center", dict(type=float, nargs=3, metavar=("X", "Y", "Z"),
                                help="the root cube's centre of --skip-tree")),
    ("--skip-carve-depth", dict(type=int, default=0)),
    ("--skip-carve-footprint", dict(choices=["point", "box"], default="point",
                                    help="--skip-carve-depth: test a cell's centre (K23) or its "
                                         "whole projected footprint (K27, conservative)")),
    ("--skip-resolution", dict(type=int, default=128)),
    ("--skip-dilate", dict(type=int, default=1)),
]
# not flags of the reference either: the focus half of every ray's samples drawn from an octree's own
# weights instead of a coarse model (DESIGN K26), from a saved octree or from one carved out of the
# training images' silhouettes at this depth (0 = off; colour "visible", no fit).  A table of its own
# like SKIP_GRID; mutually exclusive with --opacity-model
FOCUS_TREE = [
    ("--focus-tree", dict(help="octree NPZ (a density per leaf) the focus samples are drawn from")),
    ("--focus-tree-center", dict(type=float, nargs=3, metavar=("X", "Y", "Z"),
                                 help="the root cube's centre of --focus-tree")),
    ("--focus-carve-depth", dict(type=int, default=0)),
    ("--focus-carve-footprint", dict(choices=["point", "box"], default="point",
                                     help="--focus-carve-depth: test a cell's centre (K23) or its "
                                          "whole projected footprint (K27, conservative)")),
    ("--focus-min-mass", dict(type=float, default=1e-3,
                              help="rays whose tree weights sum to less sample uniformly")),
]
NERF_ONLY = [
    ("--resolution", dict(type=int, default=400)),
    ("--num-cameras", dict(type=int, default=100)),
    ("--num-layers", dict(type=int, default=8)),
    ("--pos-freq", dict(type=int, default=10)),
    ("--pos-max-log-scale", dict(type=float, default=9)),
    ("--view-freq", dict(type=int, default=4)),
    ("--view-max-log-scale", dict(type=float, default=3)),
    ("--omit-inputs", dict(action="store_true")),
    ("--decay-steps", dict(type=int, default=250000)),
]
TINY_ONLY = [
    ("--embedding-size", dict(type=int, default=256)),
    ("--pos-max-log-scale", dict(type=float, default=5.5)),
    ("--gauss-sigma", dict(type=float, default=6.05)),
    ("--make-activations", dict(action="store_true")),
    ("--decay-steps", dict(type=int, default=25000)),
]
# train_voxels.py:11-49 of the reference (positionals data_path side results_dir; --num-cameras is
# parsed but unused there too)
VOXELS = [
    ("data_path", dict(help="Path to the data NPZ")),
    ("side", dict(type=int, help="One side of the voxel volume")),
    ("results_dir", dict(help="Path to output results")),
    ("--mode", dict(choices=["rgba", "rgb", "dilate"], default="rgba")),
    ("--num-samples", dict(type=int, default=256)),
    ("--num-cameras", dict(type=int, default=100)),
    ("--batch-size", dict(type=int, default=1024)),
    ("--learning-rate", dict(type=float, default=0.01)),
    ("--num-steps", dict(type=int, default=10000)),
    ("--report-interval", dict(type=int, default=1000)),
    ("--image-interval", dict(type=int, default=2000)),
    ("--seed", dict(type=int, default=20080524)),
    ("--decay-rate", dict(type=float, default=0.9)),
    ("--decay-steps", dict(type=int, default=25000)),
    ("--make-video", dict(action="store_true")),
    ("--color-space", dict(choices=["YCrCb", "RGB"], default="RGB")),
    ("--num-frames", dict(type=int, default=200)),
    ("--device", dict(default="cuda")),
    ("--anneal-start", dict(type=float, default=0.2)),
    ("--num-anneal-steps", dict(type=int, default=2000)),
]
# train_image_regression.py:21-59 of the reference (positionals image_path nerf_model results_dir)
IMAGE_REGRESSION = [
    ("image_path", dict(help="Path to an image file")),
    ("nerf_model", dict(choices=["mlp", "basic", "positional", "gaussian"])),
    ("results_dir", dict(help="Path to the results directory")),
    ("--activations", dict(action="store_true", help="Produce activation visualizations")),
    ("--vertical", dict(action="store_true", help="Whether to stack the images vertically")),
    ("--omit-gt", dict(action="store_true", help="whether to omit the GT image from the display")),
    ("--image-size", dict(type=int, default=512, help="Size of the square input image")),
    ("--color-space", dict(choices=["YCrCb", "RGB"], default="RGB")),
    ("--num-channels", dict(type=int, default=256)),
    ("--embedding_size", dict(type=int, default=256)),
    ("--pos-max-log-scale", dict(type=float, default=6)),
    ("--gauss-sigma", dict(type=float, default=10)),
    ("--num-steps", dict(type=int, default=2000)),
    ("--learning-rate", dict(type=float, default=1e-3)),
    ("--report-interval", dict(type=int, default=50)),
    ("--make-video", dict(action="store_true")),
    ("--decay-rate", dict(type=float, default=0.1)),
    ("--decay-steps", dict(type=int, default=2500)),
    ("--device", dict(default="cuda")),
]
# train_signal_regression.py:48-78 of the reference (positionals signal results_dir; --num_plot is
# spelled with an underscore there too), then --device as in the other drivers
SIGNAL_REGRESSION = [
    ("signal", dict(choices=["multifreq", "sawtooth", "triangle"],
                    help="the 1-D signal to fit")),
    ("results_dir", dict(help="directory for log.txt and the frames")),
    ("--num-channels", dict(type=int, default=64, help="hidden channels")),
    ("--num-layers", dict(type=int, default=1, help="hidden layers")),
    ("--num-samples", dict(type=int, default=32, help="training samples")),
    ("--sample-rate", dict(type=int, default=8,
                           help="validation points per training sample")),
    ("--num_plot", dict(type=int, default=48,
                        help="points in the plots")),
    ("--max-hidden", dict(type=int, default=10,
                          help="hidden units drawn")),
    ("--fourier", dict(action="store_true", help="Fourier-feature input encoding")),
    ("--resolution", dict(default="1280x720", help="frame size WIDTHxHEIGHT")),
    ("--num-steps", dict(type=int, default=10000, help="training steps")),
    ("--make-video", dict(action="store_true", help="(no MP4 writer here: PNG frames instead)")),
    ("--framerate", dict(type=int, default=5, help="video frame rate (unused)")),
    ("--no-plot", dict(action="store_true", help="no frames")),
    ("--device", dict(default="cuda")),
]
# voxelize_model.py:11-33 of the reference (positionals model_path data_path output_path;
# --num-cameras is a float there too)
VOXELIZE = [
    ("model_path", dict(help="Path to the saved model")),
    ("data_path", dict(help="Path to the data used to train the model")),
    ("output_path", dict(help="Path to the output octree")),
    ("--scenepic-path", dict()),
    ("--voxel-depth", dict(type=int, default=8, help="Depth of the octree to use")),
    ("--num-cameras", dict(type=float, default=100,
                           help="Number of cameras to use for sampling the volume")),
    ("--batch-size", dict(type=int, default=4096, help="Number of rays to process in a batch")),
    ("--min-leaf-size", dict(type=int, default=4, help="Minimum number of samples in a leaf")),
    ("--alpha-threshold", dict(type=float, default=0.3,
                               help="Threshold to use when filtering samples")),
    ("--opacity-model-path", dict(help="Path to an optional opacity model")),
    ("--device", dict(default="cuda", help="Pytorch compute device")),
]
ORBIT = [
    ("model_path", dict(help="trained checkpoint")),
    ("resolution", dict(type=int, help="frame size in pixels")),
    ("output_dir", dict(help="directory for the PNG frames")),
    ("--opacity-model", dict(help="optional checkpoint of an opacity model")),
    ("--distance", dict(type=float, default=4)),
    ("--fov-y-degrees", dict(type=float, default=40)),
    ("--num-frames", dict(type=int, default=200)),
    ("--up-dir", dict(default="y+", choices=["x+", "x-", "y+", "y-", "z+", "z-"])),
    ("--forward-dir", dict(default="z-", choices=["x+", "x-", "y+", "y-", "z+", "z-"])),
    ("--num-samples", dict(type=int, default=128)),
    ("--alpha-thresh", dict(type=float, default=0.3)),
    ("--batch_size", dict(type=int, default=4096)),
    ("--device", dict(default="cuda")),
    ("--precision", dict(choices=["f32", "bf16x3", "bf16x6"], default="f32")),   # not a flag of the reference
    FOCUS_MODE,
]


def build_parser(title, *tables, positional_extra=()):
    parser = argparse.ArgumentParser(title, formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    flat = []
    for table in tables:
        flat.extend(table)
    pos = [row for row in flat if not row[0].startswith("-")]
    opt = [row for row in flat if row[0].startswith("-")]
    for name, kw in pos[:1] + list(positional_extra) + pos[1:] + opt:
        parser.add_argument(name, **kw)
    return parser


def setup_device(requested: str, want_group: bool):
    """Resolves --device for this process and makes it torch's current device (the C ABI
    launches on the current device).  Under ``torch.distributed.run`` (WORLD_SIZE > 1) a plain
    "cuda" becomes cuda:LOCAL_RANK and, if ``want_group``, the RCCL process group is created
    (training: gradients are all-reduced; rendering is replicas-only and needs none).
    Returns (device string, rank, world, group or None)."""
    import torch
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    device = requested
    if world > 1 and device == "cuda":
        device = "cuda:%d" % int(os.environ.get("LOCAL_RANK", "0"))
    dev = torch.device(device)
    if dev.type == "cuda":
        torch.cuda.set_device(dev if dev.index is not None else torch.device("cuda", 0))
    group = None
    if want_group and world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29500")
        backend = os.environ.get("FFN_DIST_BACKEND", "nccl")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world,
                                    device_id=torch.device("cuda", torch.cuda.current_device()))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
        group = dist.group.WORLD
    return device, rank, world, group


def apply_precision(model, precision: str):
    """--precision bf16x3 / bf16x6: the opt-in split kernels for training and inference calls of a
    fused model (bf16x3: three bf16 products per f32 product, ~2^-16 per product; bf16x6: three-part
    operands, six products, the error of an f32 dot product -- chains of <= 256 channels); the
    default is the exact-f32 kernels.  Not a flag of the reference."""
    if precision != "f32" and hasattr(model, "train_precision"):
        model.precision = precision
        model.train_precision = precision
    return model


def focus_mode(args) -> str:
    """--focus-mode for samplers whose opacity model is a frozen checkpoint: auto -> live."""
    mode = getattr(args, "focus_mode", "auto")
    return "live" if mode == "auto" else mode


def carve_footprint(args, prefix):
    """The carve arguments of --skip-carve-footprint / --focus-carve-footprint (``prefix`` "skip" or
    "focus"): nothing for "point", so that the default call stays the call it was."""
    footprint = getattr(args, "%s_carve_footprint" % prefix, "point")
    return {} if footprint == "point" else {"footprint": footprint}


def apply_skipping(caster, args, train=None):
    """--skip-empty-space: the opt-in occupancy-grid schedule of Raycaster.fit.  --skip-tree /
    --skip-carve-depth: a grid that needs no model (DESIGN K25), from a saved octree or carved
    from the training images' silhouettes, imposed from step 0.  Such a grid goes to training AND
    to rendering: a model trained under a grid has learned nothing about the cells it leaves out,
    so it must be rendered under the same grid (scripts/skip_training_demo.py)."""
    if getattr(args, "skip_empty_space", False):
        caster.train_occupancy_schedule = (args.skip_warmup, args.skip_refresh)
    tree_path = getattr(args, "skip_tree", None)
    carve_depth = getattr(args, "skip_carve_depth", 0)
    if tree_path is None and not carve_depth:
        return caster
    if tree_path is not None and carve_depth:
        raise SystemExit("--skip-tree and --skip-carve-depth are two sources of one grid: pass one")
    if train is None:
        raise SystemExit("--skip-tree / --skip-carve-depth need the training dataset")
    import fourier_feature_nets_amd as ffn
    if tree_path is not None:
        tree = ffn.OcTree.load(tree_path)
        if tree is None:
            raise SystemExit("--skip-tree: cannot read %s" % tree_path)
        if args.skip_tree_center is None:
            raise SystemExit("--skip-tree needs --skip-tree-center X Y Z: a saved tree does not "
                             "hold its root cube's centre")
        grid = ffn.OccupancyGrid.from_octree(tree, train.sampler.bounds, args.skip_resolution,
                                             center=args.skip_tree_center, dilate=args.skip_dilate)
    else:
        grid = ffn.OccupancyGrid.from_silhouettes(train, resolution=args.skip_resolution,
                                                  depth=carve_depth, dilate=args.skip_dilate,
                                                  **carve_footprint(args, "skip"))
    print("empty-space skipping from step 0: %.4f of the %d^3 cells occupied"
          % (grid.fraction_occupied(), grid.resolution))
    caster.train_occupancy = grid
    caster.occupancy = grid
    return caster


def check_focus_tree(args):
    """--focus-tree / --focus-carve-depth against each other and against --opacity-model, before
    anything is loaded."""
    tree_path = getattr(args, "focus_tree", None)
    carve_depth = getattr(args, "focus_carve_depth", 0)
    if tree_path is None and not carve_depth:
        return False
    if tree_path is not None and carve_depth:
        raise SystemExit("--focus-tree and --focus-carve-depth are two sources of one tree: pass one")
    if getattr(args, "opacity_model", None):
        raise SystemExit("--focus-tree / --focus-carve-depth and --opacity-model are two sources of "
                         "one distribution: pass one")
    if tree_path is not None and args.focus_tree_center is None:
        raise SystemExit("--focus-tree needs --focus-tree-center X Y Z: a saved tree does not hold "
                         "its root cube's centre")
    return True


def focus_tree(args, train=None):
    """The tree and centre of --focus-tree / --focus-carve-depth -> (tree, center), or None when
    neither is given.  Carving needs the training dataset: the cube is the bounds' box, the colours
    come from the cameras that see a leaf (``color="visible"``), nothing is fitted."""
    if not check_focus_tree(args):
        return None
    import fourier_feature_nets_amd as ffn
    if args.focus_tree is not None:
        tree = ffn.OcTree.load(args.focus_tree)
        if tree is None:
            raise SystemExit("--focus-tree: cannot read %s" % args.focus_tree)
        return tree, tuple(args.focus_tree_center)
    if train is None:
        raise SystemExit("--focus-carve-depth needs the training dataset")
    lo, size = ffn.OccupancyGrid.box_of(train.sampler.bounds)
    center = tuple(float(v) for v in lo + 0.5 * size)
    tree = ffn.OcTree.build_from_silhouettes(train, args.focus_carve_depth, center,
                                             0.5 * float(size.max()), color="visible",
                                             **carve_footprint(args, "focus"))
    return tree, center


def apply_focus_tree(args, train, *others):
    """Points the samplers of ``train`` and of every other dataset at the tree of --focus-tree /
    --focus-carve-depth (``RaySampler.focus_on_octree``) and prints the share of a camera's rays that
    will sample from it (mass >= --focus-min-mass); without the options nothing changes."""
    found = focus_tree(args, train)
    if found is None:
        return None
    tree, center = found
    for ds in (train,) + others:
        ds.sampler = ds.sampler.focus_on_octree(tree, center, args.focus_min_mass)
    report_focus_share(train.sampler)
    return tree


def report_focus_share(sampler, camera: int = 0):
    rays = sampler._valid_for_camera(camera)
    if rays.numel() == 0:
        return
    mass = sampler.focus_mass(rays)
    share = float((mass >= sampler.focus_min_mass).float().mean())
    print("focus samples from an octree of %d leaves: %.4f of camera %d's %d rays have mass >= %g "
          "(the others sample uniformly)" % (sampler.focus_tree.num_leaves, share, camera,
                                             rays.numel(), sampler.focus_min_mass))


def axis_vector(code):
    vec = np.zeros(3, np.float32)
    vec["xyz".index(code[0])] = 1 if code[1] == "+" else -1
    return vec


def write_log(path, args, log):
    """log.txt in the reference layout: the args as JSON, a blank line, a tab-separated
    header and one row per report."""
    with open(path, "w") as f:
        json.dump(vars(args), f)
        f.write("\n\n")
        f.write("\t".join(["step", "timestamp", "psnr_train", "psnr_val"]) + "\n")
        for e in log:
            f.write("\t".join(str(v) for v in (e.step, e.timestamp, e.train_psnr, e.val_psnr)) + "\n")


def save_png(path, image):
    from PIL import Image
    Image.fromarray(image).save(path)
