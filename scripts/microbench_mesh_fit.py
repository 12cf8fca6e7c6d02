"""Microbenchmark of K32, the backward of ``mesh.render_mesh`` in the vertex colours, on the K30
meshes of ``scripts/microbench_octree_mesh.py`` (surface nets of the depth-8 and depth-10 density
trees of the opaque ball) at 400 x 400, next to K31's frame time of
``profiles/r29_mesh_raster_microbench.json`` for scale.

Times, in one process, best of ``--repeats`` after a warm-up call:

* K32a (face sums) and K32b (vertex gather) between device events, one camera;
* one ``render_mesh_backward`` (K31a-c for the ids, K32a, K32b) between device events and as wall
  time, the adjacency made beforehand;
* ``vertex_adjacency`` (a torch stable sort) as wall time;
* one step of ``fit_mesh_colors`` with one camera per step, as wall time: the difference of a fit
  of ``1 + --fit-steps`` steps and a fit of 1 step, divided by ``--fit-steps``;
* ``color_mesh_from_images`` over ``--cameras`` cameras as wall time.

The targets are K31's own frames of the mesh with its K30 colours.  No time is gated and nothing is
tuned after the result.  Kernel times under rocprofv3 are not collected.

    python scripts/microbench_mesh_fit.py [--repeats 5] [--out profiles/r30_mesh_fit_microbench.json]
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
from fourier_feature_nets_amd import mesh as mesh_module  # noqa: E402
from fourier_feature_nets_amd import ops  # noqa: E402
from scripts.microbench_mesh_raster import on_gpu, rig  # noqa: E402
from scripts.microbench_octree_carve import quiet  # noqa: E402
from scripts.microbench_octree_render import device_ms  # noqa: E402
from scripts.microbench_octree_walk import opaque_ball, wall  # noqa: E402

DEFAULT_OUT = os.path.join(ROOT, "profiles", "r30_mesh_fit_microbench.json")
K31_PROFILE = os.path.join(ROOT, "profiles", "r29_mesh_raster_microbench.json")


def k31_for_scale(name):
    """The stage times K31's microbenchmark recorded for the same mesh, or None."""
    try:
        with open(K31_PROFILE) as f:
            cases = json.load(f)["cases"]
    except (OSError, ValueError, KeyError):
        return None
    for case in cases:
        if case.get("mesh") == name:
            return {key: case[key] for key in case if key.endswith("_ms")}
    return None


def frames_of(surface, cameras):
    size = cameras[0].resolution.width
    images = np.zeros((len(cameras), size, size, 4), np.uint8)
    for index, camera in enumerate(cameras):
        color, alpha, _ = ffn.render_mesh_image(surface.vertices, surface.triangles, camera,
                                                colors=surface.colors, include_depth=True)
        images[index, ..., :3] = color
        images[index, ..., 3] = np.rint(255 * alpha)
    return images


def fit_case(surface, cameras, args):
    camera = cameras[0]
    width, height = camera.resolution
    proj = ffn.projection_matrices([camera])[0]
    eye = ffn.eye_positions([camera], (0.0, 0.0, 0.0))[0]
    v, t = on_gpu(surface.vertices, "float32"), on_gpu(surface.triangles, "int32")
    c = on_gpu(surface.colors, "float32")
    repeats = args.repeats
    out = {"vertices": len(surface.vertices), "triangles": len(surface.triangles)}
    out["vertex_adjacency_wall_ms"] = wall(lambda: mesh_module.vertex_adjacency(t, len(v)),
                                           repeats)[0]
    order, starts = mesh_module.vertex_adjacency(t, len(v))
    out["largest_valence"] = int((starts[1:] - starts[:-1]).max().item())
    record = ops.mesh_raster_setup(v, t, proj, width, height)[0]
    color, alpha, _, ids, _, total = mesh_module.rasterize_mesh(v, t, proj, eye, width, height, c)
    out["box_pixels"] = total
    out["covered_share_of_the_image"] = float(alpha.mean().item())
    d_color = torch.randn((width * height, 3), device="cuda",
                          generator=torch.Generator(device="cuda").manual_seed(1))
    out["k32a_face_sums_device_ms"] = device_ms(
        lambda: ops.mesh_raster_face_sums(record, ids, d_color, width, height), repeats)
    sums = ops.mesh_raster_face_sums(record, ids, d_color, width, height)
    grad = torch.empty((len(v), 3), device="cuda")
    weight = torch.empty((len(v),), device="cuda")
    out["k32b_vertex_gather_device_ms"] = device_ms(
        lambda: ops.mesh_vertex_gather(sums, order, starts, grad, weight), repeats)

    def backward():
        return ffn.render_mesh_backward(v, t, camera, d_color, (order, starts), grad, weight)
    out["render_mesh_backward_device_ms"] = device_ms(backward, repeats)
    out["render_mesh_backward_wall_ms"] = wall(backward, repeats)[0]
    out["render_mesh_wall_ms"] = wall(lambda: ffn.render_mesh(v, t, camera, colors=c), repeats)[0]

    images = frames_of(surface, cameras)
    bounds = np.diag([2, 2, 2, 1]).astype(np.float32)
    train = quiet(ffn.ImageDataset, "train", images, bounds, cameras, 8, device="cuda")
    grey = torch.full((len(v), 3), 0.5, device="cuda")

    def fit(steps):
        return ffn.fit_mesh_colors(v, t, grey, train, num_steps=steps, verbose=False)
    one = wall(lambda: fit(1), repeats)[0]
    many, (_, log) = wall(lambda: fit(1 + args.fit_steps), repeats)
    out["fit_steps_timed"] = args.fit_steps
    out["fit_step_wall_ms"] = (many - one) / args.fit_steps
    out["fit_loss_first_last"] = [log[0].loss, log[-1].loss]
    out["color_mesh_from_images_cameras"] = len(cameras)
    out["color_mesh_from_images_wall_ms"], (_, weights) = wall(
        lambda: ffn.color_mesh_from_images(v, t, train), repeats)
    out["vertices_seen"] = int((weights > 0).sum().item())
    return out


def main():
    parser = argparse.ArgumentParser()
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
    for depth in args.depths:
        tree = ffn.OcTree.build_from_model(model, depth, alpha_threshold=0.01)
        surface = tree.extract_mesh(0.01)
        name = "extract_mesh(0.01, surface_nets) of the depth-%d density tree" % depth
        case = {"mesh": name}
        case.update(fit_case(surface, cameras, args))
        case["k31_for_scale"] = k31_for_scale(name)
        results["cases"].append(case)
        print(json.dumps(case), flush=True)
        write()
        del tree, surface
        torch.cuda.empty_cache()
    results["complete"] = True
    write()
    return 0


if __name__ == "__main__":
    sys.exit(main())
