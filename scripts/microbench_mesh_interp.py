"""Microbenchmark of K35 -- the interior half of the geometry gradient, colour through the
barycentric weights -- in the setting of ``scripts/microbench_mesh_aa.py``: the K30 meshes of the
opaque ball (surface nets of the depth-8 and depth-10 density trees) at 400 x 400.

Times, in one process, best of ``--repeats`` after a warm-up call:

* K35a and K35b next to K32a and K32b on the same frame and the same gradient, between device
  events: K35a is K32a's loop with nine folded terms instead of twelve, so K32a is its yardstick;
* ``render_mesh_geometry_backward`` with and without ``interior``, between device events;
* one step of ``fit_mesh_geometry`` with and without ``interior``, one camera per step, as wall
  time: the difference of a fit of ``1 + --fit-steps`` steps and a fit of 1 step, divided by
  ``--fit-steps``.

No time is gated and nothing is tuned after the result.

``--quality`` runs K34's experiment again, by its protocol (``scripts/microbench_mesh_aa.py``):
the depth-8 K30 mesh of the torus' colour tree, the colours fitted to the images, then for every
learning rate of ``--geometry-rates`` and every weight of ``--laplacian-weights``
``fit_mesh_geometry`` with ``interior`` off and on, the colours taken and fitted again, and the
held-out PSNR and silhouette IoU of each arm.  The grid is K34's, fixed beforehand.

    python scripts/microbench_mesh_interp.py [--quality] [--out profiles/r33_mesh_interp_microbench.json]
"""

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import fourier_feature_nets_amd as ffn  # noqa: E402
from fourier_feature_nets_amd import fit_loop  # noqa: E402
from fourier_feature_nets_amd import mesh as mesh_module  # noqa: E402
from fourier_feature_nets_amd import ops  # noqa: E402
from scripts.microbench_mesh_fit import frames_of  # noqa: E402
from scripts.microbench_mesh_raster import mesh_frames, on_gpu, rig  # noqa: E402
from scripts.microbench_octree_carve import quiet  # noqa: E402
from scripts.microbench_octree_render import device_ms  # noqa: E402
from scripts.microbench_octree_walk import opaque_ball, wall  # noqa: E402

DEFAULT_OUT = os.path.join(ROOT, "profiles", "r33_mesh_interp_microbench.json")


def interp_case(surface, cameras, args):
    camera = cameras[0]
    width, height = camera.resolution
    proj = ffn.projection_matrices([camera])[0]
    eye = ffn.eye_positions([camera], (0.0, 0.0, 0.0))[0]
    v, t = on_gpu(surface.vertices, "float32"), on_gpu(surface.triangles, "int32")
    c = on_gpu(surface.colors, "float32")
    repeats = args.repeats
    out = {"vertices": len(surface.vertices), "triangles": len(surface.triangles)}
    record, color, alpha, _, ids, _, total, zbuf = mesh_module._rasterize_z(
        v, t, proj, eye, width, height, c)
    out["box_pixels"] = total
    out["covered_share_of_the_image"] = float(alpha.mean().item())
    out["triangles_that_win_a_pixel"] = int(torch.unique(ids[ids >= 0]).numel())
    generator = torch.Generator(device="cuda").manual_seed(1)
    g_color = torch.randn((width * height, 3), device="cuda", generator=generator)
    g_alpha = torch.randn((width * height,), device="cuda", generator=generator)
    order, starts = mesh_module.vertex_adjacency(t, len(v))
    opposite = mesh_module.edge_opposites(t, len(v))
    grad = torch.empty((len(v), 3), device="cuda")
    weight = torch.empty((len(v),), device="cuda")

    out["k32a_face_sums_device_ms"] = device_ms(
        lambda: ops.mesh_raster_face_sums(record, ids, g_color, width, height), repeats)
    sums = ops.mesh_raster_face_sums(record, ids, g_color, width, height)
    out["k32b_vertex_gather_device_ms"] = device_ms(
        lambda: ops.mesh_vertex_gather(sums, order, starts, grad, weight), repeats)
    out["k35a_face_grads_device_ms"] = device_ms(
        lambda: ops.mesh_interp_face_grads(record, ids, g_color, c, t, width, height), repeats)
    face_grads = ops.mesh_interp_face_grads(record, ids, g_color, c, t, width, height)
    out["k35b_vertex_grad_device_ms"] = device_ms(
        lambda: ops.mesh_interp_vertex_grad(face_grads, order, starts, v, proj, grad), repeats)
    out["k35a_over_k32a"] = out["k35a_face_grads_device_ms"] / out["k32a_face_sums_device_ms"]
    out["k35b_over_k32b"] = out["k35b_vertex_grad_device_ms"] / out["k32b_vertex_gather_device_ms"]

    for interior in (False, True):
        def backward():
            return ffn.render_mesh_geometry_backward(v, t, camera, c, g_color, g_alpha, opposite,
                                                     grad, interior=interior,
                                                     adjacency=(order, starts))
        key = "render_mesh_geometry_backward%s" % ("_interior" if interior else "")
        out[key + "_device_ms"] = device_ms(backward, repeats)
        out[key + "_wall_ms"] = wall(backward, repeats)[0]

    images = frames_of(surface, cameras)
    bounds = np.diag([2, 2, 2, 1]).astype(np.float32)
    train = quiet(ffn.ImageDataset, "train", images, bounds, cameras, 8, device="cuda")

    def step_ms(fit):
        one = wall(lambda: fit(1), repeats)[0]
        many, (_, log) = wall(lambda: fit(1 + args.fit_steps), repeats)
        return (many - one) / args.fit_steps, [log[0].loss, log[-1].loss]

    out["fit_steps_timed"] = args.fit_steps
    for interior in (False, True):
        key = "fit_mesh_geometry%s" % ("_interior" if interior else "")
        out[key + "_step_wall_ms"], out[key + "_loss_first_last"] = step_ms(
            lambda steps: ffn.fit_mesh_geometry(v, t, c, train, num_steps=steps, verbose=False,
                                                interior=interior))
    return out


def quality(args, write, out):
    """K34's experiment with ``interior`` off and on.  ``out`` is filled arm by arm and written
    after each."""
    mesh = ffn.procedural_torus()
    points = ffn.normalize_points(mesh[0])
    cameras = rig(args.quality_cameras, args.size)
    images = mesh_frames(points, mesh[1], mesh[2], mesh[3], cameras, 1)
    n_val, n_test = max(1, len(cameras) // 17), max(1, len(cameras) // 9)
    n_train = len(cameras) - n_val - n_test
    bounds = np.diag([2, 2, 2, 1]).astype(np.float32)
    train = quiet(ffn.ImageDataset, "train", images[:n_train], bounds, cameras[:n_train], 8,
                  device="cuda")
    held = quiet(ffn.ImageDataset, "held", images[n_train:], bounds, cameras[n_train:], 8,
                 device="cuda")
    held_cameras = cameras[n_train:]
    truth = [torch.from_numpy(images[n_train + k][..., 3].reshape(-1) >= 128).cuda()
             for k in range(len(held_cameras))]
    tree = ffn.OcTree.build_from_triangles(*mesh, args.quality_depth, 4)
    surface = tree.extract_mesh()
    out.update({
        "data": "procedural_torus() drawn by K31 at %d x %d from the %d cameras of "
                "make_mesh_npz.py --render mesh; %d train, %d held out (val and test)"
                % (args.size, args.size, len(cameras), n_train, n_val + n_test),
        "mesh": "extract_mesh() of the depth-%d colour tree of the torus" % args.quality_depth,
        "vertices": len(surface.vertices), "triangles": len(surface.triangles),
        "color_steps": args.quality_steps, "color_learning_rate": args.learning_rate,
        "geometry_steps": args.quality_steps, "cameras_per_step": args.cameras_per_step,
        "psnr": "-10 log10 of the mean colour MSE over all pixels of the held-out cameras, K31's "
                "plain picture (no antialiasing)",
        "iou": "mean over the held-out cameras of |drawn & truth| / |drawn | truth|, truth where "
               "the image's alpha byte is 128 or more", "arms": []})
    t = on_gpu(surface.triangles, "int32")
    start = on_gpu(surface.vertices, "float32")

    def measure(v, colors):
        frame = mesh_module._color_frames(v, t, colors, held_cameras, args.size, args.size)
        ious = []
        for number in range(len(held_cameras)):
            drawn = frame(number)[2][1] >= 0
            union = int((drawn | truth[number]).sum().item())
            ious.append(int((drawn & truth[number]).sum().item()) / max(union, 1))
        return (fit_loop.camera_psnr(frame, len(held_cameras), args.size * args.size, held),
                float(np.mean(ious)))

    def colour(v):
        colors, _ = ffn.color_mesh_from_images(v, t, train, on_gpu(surface.colors, "float32"))
        colors, log = ffn.fit_mesh_colors(v, t, colors, train, num_steps=args.quality_steps,
                                          learning_rate=args.learning_rate,
                                          cameras_per_step=args.cameras_per_step, verbose=False)
        return colors, [log[0].loss, log[-1].loss]

    colors, losses = colour(start)
    out["a_fitted_colors_psnr"], out["a_fitted_colors_iou"] = measure(start, colors)
    out["a_color_fit_loss_first_last"] = losses
    write()
    for rate in args.geometry_rates:
        for weight in args.laplacian_weights:
            for interior in (False, True):
                fitted, log = ffn.fit_mesh_geometry(
                    start, t, colors, train, num_steps=args.quality_steps, learning_rate=rate,
                    cameras_per_step=args.cameras_per_step, laplacian_weight=weight,
                    verbose=False, interior=interior)
                moved = (fitted - start).norm(dim=1)
                finite = bool(torch.isfinite(fitted).all().item())
                arm = {"learning_rate": rate, "laplacian_weight": weight, "interior": interior,
                       "geometry_loss_first_last": [log[0].loss, log[-1].loss],
                       "geometry_loss_mean_first10_last10": [
                           float(np.mean([e.loss for e in log[:10]])),
                           float(np.mean([e.loss for e in log[-10:]]))],
                       "mean_displacement": float(moved.mean().item()),
                       "largest_displacement": float(moved.max().item()),
                       "vertices_that_moved_share": float((moved > 0).float().mean().item()),
                       "finite": finite}
                if finite:
                    arm["old_colors_psnr"], arm["old_colors_iou"] = measure(fitted, colors)
                    again, losses = colour(fitted)
                    arm["refitted_colors_psnr"], arm["refitted_colors_iou"] = measure(fitted, again)
                    arm["color_refit_loss_first_last"] = losses
                    del again
                out["arms"].append(arm)
                print(json.dumps(arm), flush=True)
                write()
                del fitted
    return out


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--quality", action="store_true")
    parser.add_argument("--quality-only", action="store_true")
    parser.add_argument("--quality-cameras", type=int, default=120)
    parser.add_argument("--quality-depth", type=int, default=8)
    parser.add_argument("--quality-steps", type=int, default=300)
    parser.add_argument("--learning-rate", type=float, default=1e-2,
                        help="of the colour fits, K33's")
    parser.add_argument("--cameras-per-step", type=int, default=4)
    parser.add_argument("--geometry-rates", type=float, nargs="*", default=[1e-4, 1e-3, 1e-2])
    parser.add_argument("--laplacian-weights", type=float, nargs="*", default=[0.0, 1e2, 1e4])
    parser.add_argument("--repeats", type=int, default=5)
    parser.add_argument("--depths", type=int, nargs="*", default=[8, 10])
    parser.add_argument("--size", type=int, default=400)
    parser.add_argument("--cameras", type=int, default=8)
    parser.add_argument("--fit-steps", type=int, default=20)
    parser.add_argument("--out", default=DEFAULT_OUT)
    args = parser.parse_args()
    results = {"device": torch.cuda.get_device_name(0), "frame": [args.size, args.size],
               "repeats": args.repeats, "precision": "f32 and integers (no matrix work on this path)",
               "rocprofv3_kernel_times": "not collected", "cases": [], "complete": False}

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(results, indent=1) + "\n")

    cameras = rig(args.cameras, args.size)
    model = opaque_ball()
    for depth in ([] if args.quality_only else args.depths):
        tree = ffn.OcTree.build_from_model(model, depth, alpha_threshold=0.01)
        surface = tree.extract_mesh(0.01)
        case = {"mesh": "extract_mesh(0.01, surface_nets) of the depth-%d density tree" % depth}
        case.update(interp_case(surface, cameras, args))
        results["cases"].append(case)
        print(json.dumps(case), flush=True)
        write()
        del tree, surface
        torch.cuda.empty_cache()
    if args.quality or args.quality_only:
        results["quality"] = {}
        quality(args, write, results["quality"])
    results["complete"] = True
    write()
    return 0


if __name__ == "__main__":
    sys.exit(main())
