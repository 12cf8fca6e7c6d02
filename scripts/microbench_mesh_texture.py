"""Microbenchmark of K33, the textured picture of a mesh as a sparse matrix in its texture, on the
K30 meshes of ``scripts/microbench_mesh_fit.py`` (surface nets of the depth-8 and depth-10 density
trees of the opaque ball, the shapes of ``profiles/r30_mesh_fit_microbench.json``) unwrapped with
``--tiles`` 4 and 8, at 400 x 400; and the quality experiment K31 and K32 left unmeasured.

Times, in one process, best of ``--repeats`` after a warm-up call:

* K33a (taps), K33b (forward gather) and K33c (transposed gather) between device events, one camera;
* the stable sort of the tap slots between device events;
* ``mesh_texture_taps`` (K31a-c, K33a, the sort) and ``unwrap_mesh`` as wall time;
* one cached step of ``fit_mesh_texture`` with one camera per step, as wall time: the difference of
  a fit of ``cameras + --fit-steps`` steps and a fit of ``cameras`` steps (the first deal builds
  every camera's taps), divided by ``--fit-steps``;
* the longest and the mean texel row of the camera (over the texels that have one).

The quality experiment (``--quality-steps`` > 0): the procedural torus drawn by K31 from the cameras
of ``make_mesh_npz.py --render mesh`` (its split), the depth-8 K30 mesh of the torus' colour tree,
and the PSNR over all pixels of the held-out (val and test) cameras of (a) K30's colours, (b)
``color_mesh_from_images`` + ``fit_mesh_colors``, (c) ``texture_mesh_from_images`` +
``fit_mesh_texture`` at every tile.  No time is gated and nothing is tuned after the result.

    python scripts/microbench_mesh_texture.py [--repeats 5] [--out profiles/r31_mesh_texture_microbench.json]
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

DEFAULT_OUT = os.path.join(ROOT, "profiles", "r31_mesh_texture_microbench.json")
BOUNDS = np.diag([2, 2, 2, 1]).astype(np.float32)


def texture_case(surface, cameras, train, tile, args):
    camera = cameras[0]
    width, height = camera.resolution
    repeats = args.repeats
    out = {"tile": tile}
    out["unwrap_mesh_wall_ms"], unwrapped = wall(
        lambda: ffn.unwrap_mesh(surface.vertices, surface.triangles, tile), 1)
    vertices, triangles, uvs, _, size = unwrapped
    num_texels = size[0] * size[1]
    out.update(vertices=len(vertices), triangles=len(triangles), texture=[size[1], size[0]],
               texels=num_texels)
    v, t, uv = on_gpu(vertices, "float32"), on_gpu(triangles, "int32"), on_gpu(uvs, "float32")
    proj = ffn.projection_matrices([camera])[0]
    record, ids = mesh_module._raster_ids(v, t, proj, width, height, 1 << 22)
    out["covered_share_of_the_image"] = float((ids >= 0).float().mean().item())

    def taps():
        return ops.mesh_texture_taps(record, ids, t, uv, size[0], size[1], width, height)
    out["k33a_taps_device_ms"] = device_ms(taps, repeats)
    tap_texel, tap_weight = taps()
    out["sort_device_ms"] = device_ms(
        lambda: torch.sort(tap_texel.reshape(-1), stable=True), repeats)
    out["mesh_texture_taps_wall_ms"], made = wall(
        lambda: ffn.mesh_texture_taps(v, t, uv, camera, size), repeats)
    texture = torch.rand((num_texels, 3), device="cuda",
                         generator=torch.Generator(device="cuda").manual_seed(2))
    d_color = torch.randn((width * height, 3), device="cuda",
                          generator=torch.Generator(device="cuda").manual_seed(1))
    out["k33b_gather_device_ms"] = device_ms(
        lambda: ops.mesh_texture_gather(made.tap_texel, made.tap_weight, texture), repeats)
    grad = torch.empty((num_texels, 3), device="cuda")
    weight = torch.empty((num_texels,), device="cuda")
    out["k33c_grad_device_ms"] = device_ms(
        lambda: ops.mesh_texture_grad(made.sorted_texels, made.tap_order, made.tap_weight, d_color,
                                      num_texels, grad, weight), repeats)
    rows = torch.bincount(made.sorted_texels[made.sorted_texels >= 0].to(torch.int64),
                          minlength=num_texels)
    out["longest_texel_row"] = int(rows.max().item())
    out["texels_with_a_row"] = int((rows > 0).sum().item())
    out["mean_texel_row"] = float(rows.sum().item()) / max(out["texels_with_a_row"], 1)
    del made, grad, weight, texture, d_color, rows
    torch.cuda.empty_cache()

    grey = torch.full(size + (3,), 0.5, device="cuda")

    def fit(steps):
        return ffn.fit_mesh_texture(v, t, uv, grey, train, num_steps=steps, verbose=False)
    first = len(cameras)
    base = wall(lambda: fit(first), repeats)[0]
    many, (_, log) = wall(lambda: fit(first + args.fit_steps), repeats)
    out["fit_steps_timed"] = args.fit_steps
    out["cached_fit_step_wall_ms"] = (many - base) / args.fit_steps
    out["fit_loss_first_last"] = [log[0].loss, log[-1].loss]
    return out


def quality(args):
    """Held-out PSNR of K30's colours, fitted vertex colours and fitted textures on the torus."""
    mesh = ffn.procedural_torus()
    points = ffn.normalize_points(mesh[0])
    cameras = rig(args.quality_cameras, args.size)
    images = mesh_frames(points, mesh[1], mesh[2], mesh[3], cameras, 1)
    n_val, n_test = max(1, len(cameras) // 17), max(1, len(cameras) // 9)
    n_train = len(cameras) - n_val - n_test
    train = quiet(ffn.ImageDataset, "train", images[:n_train], BOUNDS, cameras[:n_train], 8,
                  device="cuda")
    held = quiet(ffn.ImageDataset, "held", images[n_train:], BOUNDS, cameras[n_train:], 8,
                 device="cuda")
    held_cameras = cameras[n_train:]
    tree = ffn.OcTree.build_from_triangles(*mesh, args.quality_depth, 4)
    surface = tree.extract_mesh()
    out = {"data": "procedural_torus() drawn by K31 at %d x %d from the %d cameras of "
                   "make_mesh_npz.py --render mesh; %d train, %d held out (val and test)"
                   % (args.size, args.size, len(cameras), n_train, n_val + n_test),
           "mesh": "extract_mesh() of the depth-%d colour tree of the torus" % args.quality_depth,
           "vertices": len(surface.vertices), "triangles": len(surface.triangles),
           "steps": args.quality_steps, "learning_rate": args.learning_rate,
           "cameras_per_step": args.cameras_per_step,
           "psnr": "-10 log10 of the mean colour MSE over all pixels of the held-out cameras"}
    v, t = on_gpu(surface.vertices, "float32"), on_gpu(surface.triangles, "int32")
    c = on_gpu(surface.colors, "float32")

    def vertex_psnr(colors):
        frame = mesh_module._color_frames(v, t, colors, held_cameras, args.size, args.size)
        return fit_loop.camera_psnr(frame, len(held_cameras), args.size * args.size, held)
    out["a_k30_colors_psnr"] = vertex_psnr(c)
    colors, _ = ffn.color_mesh_from_images(v, t, train, c)
    out["b_color_mesh_from_images_psnr"] = vertex_psnr(colors)
    colors, log = ffn.fit_mesh_colors(v, t, colors, train, num_steps=args.quality_steps,
                                      learning_rate=args.learning_rate,
                                      cameras_per_step=args.cameras_per_step, verbose=False)
    out["b_fit_mesh_colors_psnr"] = vertex_psnr(colors)
    out["b_fit_loss_first_last"] = [log[0].loss, log[-1].loss]
    del colors
    for tile in args.tiles:
        vertices, triangles, uvs, vertex_map, size = ffn.unwrap_mesh(surface.vertices,
                                                                     surface.triangles, tile)
        tv, tt, tuv = (on_gpu(vertices, "float32"), on_gpu(triangles, "int32"),
                       on_gpu(uvs, "float32"))
        held_taps = [ffn.mesh_texture_taps(tv, tt, tuv, camera, size) for camera in held_cameras]

        def texture_psnr(texture):
            flat = texture.reshape(-1, 3)

            def frame(number):
                return ops.mesh_texture_gather(held_taps[number].tap_texel,
                                               held_taps[number].tap_weight, flat)
            return fit_loop.camera_psnr(frame, len(held_taps), args.size * args.size, held)
        start = on_gpu(ffn.bake_vertex_colors(surface.colors[vertex_map], triangles, uvs, size,
                                              tile), "float32")
        key = "c_tile_%d" % tile
        out[key + "_texture"] = [size[1], size[0]]
        out[key + "_baked_k30_colors_psnr"] = texture_psnr(start)
        texture, weights = ffn.texture_mesh_from_images(tv, tt, tuv, train, size, start)
        out[key + "_texels_seen"] = int((weights > 0).sum().item())
        out[key + "_texture_mesh_from_images_psnr"] = texture_psnr(texture)
        texture, log = ffn.fit_mesh_texture(tv, tt, tuv, texture, train,
                                            num_steps=args.quality_steps,
                                            learning_rate=args.learning_rate,
                                            cameras_per_step=args.cameras_per_step, verbose=False)
        out[key + "_fit_mesh_texture_psnr"] = texture_psnr(texture)
        out[key + "_fit_loss_first_last"] = [log[0].loss, log[-1].loss]
        del held_taps, texture, weights, start
        torch.cuda.empty_cache()
    return out


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--repeats", type=int, default=5)
    parser.add_argument("--depths", type=int, nargs="*", default=[8, 10])
    parser.add_argument("--tiles", type=int, nargs="*", default=[4, 8])
    parser.add_argument("--size", type=int, default=400)
    parser.add_argument("--cameras", type=int, default=8)
    parser.add_argument("--fit-steps", type=int, default=20)
    parser.add_argument("--quality-steps", type=int, default=300)
    parser.add_argument("--quality-cameras", type=int, default=120)
    parser.add_argument("--quality-depth", type=int, default=8)
    parser.add_argument("--learning-rate", type=float, default=1e-2, help="untuned")
    parser.add_argument("--cameras-per-step", type=int, default=4)
    parser.add_argument("--out", default=DEFAULT_OUT)
    args = parser.parse_args()
    results = {"device": torch.cuda.get_device_name(0), "frame": [args.size, args.size],
               "repeats": args.repeats, "precision": "f32 and integers (no matrix work on this path)",
               "rocprofv3_kernel_times": "not collected", "gated": "nothing: K33 has no parent",
               "cases": [], "quality": None, "complete": False}

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(results, indent=1) + "\n")

    cameras = rig(args.cameras, args.size)
    model = opaque_ball()
    for depth in args.depths:
        tree = ffn.OcTree.build_from_model(model, depth, alpha_threshold=0.01)
        surface = tree.extract_mesh(0.01)
        train = quiet(ffn.ImageDataset, "train", frames_of(surface, cameras), BOUNDS, cameras, 8,
                      device="cuda")
        name = "extract_mesh(0.01, surface_nets) of the depth-%d density tree" % depth
        for tile in args.tiles:
            case = {"mesh": name}
            case.update(texture_case(surface, cameras, train, tile, args))
            results["cases"].append(case)
            print(json.dumps(case), flush=True)
            write()
        del tree, surface, train
        torch.cuda.empty_cache()
    del model
    if args.quality_steps > 0:
        results["quality"] = quality(args)
        print(json.dumps(results["quality"]), flush=True)
    results["complete"] = True
    write()
    return 0


if __name__ == "__main__":
    sys.exit(main())
