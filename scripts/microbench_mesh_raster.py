"""Microbenchmark of K31, ``mesh.render_mesh``: the stages of the rasteriser next to the first-hit
walk of the corresponding octrees, for scale, and the octree experiments of the README measured
against frames of the mesh itself instead of frames of a voxel tree.

Times, in one process, best of ``--repeats`` after a warm-up call, one 400 x 400 camera of the
synthetic rig:

* the procedural torus (4 096 triangles, textured) next to ``OcTree.render`` / ``render_image`` of
  the K22 depth-8 tree of the same torus;
* the K30 meshes (surface nets, vertex colours) of the density trees of
  ``scripts/microbench_octree_mesh.py`` at ``--depths`` next to the first-hit frames of those trees;
* per mesh: K31a (set-up), the scan (``torch.cumsum`` and its read-back), K31b (draw), K31c
  (resolve) between device events, the whole ``render_mesh_image`` as wall time, box pixels per
  second of K31b, and the summed triangle area over the box pixels (the share of K31b's threads
  whose pixel is covered, up to the triangles that leave the image).

Quality (``--skip-quality`` leaves it out), K23's protocol: the torus, depth 8, all but the last 4
cameras to build from, those 4 held out, every pixel of theirs, black background.  Per ground truth
-- the depth-9 voxel frames of ``make_mesh_npz.py --render octree``, and ``--render mesh`` with
``--supersample`` 1 and 4 -- the carved tree as built, after 300 ``fit_octree`` steps, the K22
depth-8 tree, and the fitted tree's ``extract_mesh`` with ``corners`` and with ``surface_nets``
drawn by K31.  Nothing here asserts a number, and nothing is tuned after the result.  Kernel times
under rocprofv3 are not collected.  The result is written after every section.

    python scripts/microbench_mesh_raster.py [--repeats 5] [--out profiles/r29_mesh_raster_microbench.json]
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
from scripts.microbench_octree_carve import FIT_STEPS, HELD_OUT, psnr_all_pixels, quiet  # noqa: E402
from scripts.microbench_octree_render import device_ms  # noqa: E402
from scripts.microbench_octree_walk import opaque_ball, wall  # noqa: E402

DEFAULT_OUT = os.path.join(ROOT, "profiles", "r29_mesh_raster_microbench.json")


def on_gpu(x, dtype):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).cuda()


def raster_case(vertices, triangles, camera, repeats, colors=None, uvs=None, texture=None):
    """Stage times of one frame of a mesh (numpy arrays; the texture with row 0 at the top)."""
    width, height = camera.resolution
    proj = ffn.projection_matrices([camera])[0]
    eye = ffn.eye_positions([camera], (0.0, 0.0, 0.0))[0]
    v, t = on_gpu(vertices, "float32"), on_gpu(triangles, "int32")
    c, uv = on_gpu(colors, "float32"), on_gpu(uvs, "float32")
    tex = None if texture is None else on_gpu(np.asarray(texture)[::-1], "uint8")
    out = {"vertices": len(vertices), "triangles": len(triangles)}
    out["k31a_setup_device_ms"] = device_ms(
        lambda: ops.mesh_raster_setup(v, t, proj, width, height), repeats)
    record, status, counts = ops.mesh_raster_setup(v, t, proj, width, height)
    out["scan_device_ms"] = device_ms(lambda: ops.mesh_raster_offsets(counts), repeats)
    offsets, total = ops.mesh_raster_offsets(counts)
    tally = torch.bincount(status.to(torch.int64), minlength=len(ops.MESH_RASTER_STATUS))
    out["status"] = dict(zip(ops.MESH_RASTER_STATUS, tally.cpu().tolist()))
    out["box_pixels"] = total
    zbuf = torch.empty((width * height,), dtype=torch.int64, device="cuda")

    def draw():
        zbuf.fill_(ops.MESH_RASTER_EMPTY)
        return ops.mesh_raster_draw(record, offsets, 0, total, width, height, zbuf)
    fill = device_ms(lambda: zbuf.fill_(ops.MESH_RASTER_EMPTY), repeats)
    out["zbuf_fill_device_ms"] = fill
    out["k31b_draw_device_ms"] = device_ms(draw, repeats) - fill
    out["k31b_box_pixels_per_second"] = total / max(out["k31b_draw_device_ms"], 1e-6) * 1e3
    draw()
    out["k31c_resolve_device_ms"] = device_ms(
        lambda: ops.mesh_raster_resolve(zbuf, record, v, t, c, uv, tex, eye, (0, 0, 0), width,
                                        height), repeats)
    alpha = ops.mesh_raster_resolve(zbuf, record, v, t, c, uv, tex, eye, (0, 0, 0), width,
                                    height)[1]
    out["covered_share_of_the_image"] = float(alpha.mean().item())
    x = record[:, [0, 2, 4]].to(torch.int64)
    y = record[:, [1, 3, 5]].to(torch.int64)
    area = ((x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (y[:, 1] - y[:, 0]) * (x[:, 2] - x[:, 0]))
    pixels = float(area[status == 0].abs().sum().item()) / (2.0 * 65536.0)
    out["triangle_area_over_box_pixels"] = pixels / max(total, 1)
    paint = dict(colors=colors) if colors is not None else dict(uvs=uvs, texture=texture)
    out["render_mesh_image_wall_ms"] = wall(
        lambda: ffn.render_mesh_image(vertices, triangles, camera, **paint), repeats)[0]
    return out


def first_hit_case(tree, sampler, repeats):
    shift = torch.tensor(tree.center, dtype=torch.float32, device="cuda")
    starts = (sampler.starts[:sampler.rays_per_camera] - shift).contiguous()
    directions = sampler.directions[:sampler.rays_per_camera].contiguous()
    return {"leaves": tree.num_leaves, "depth": tree.depth,
            "first_hit_render_device_ms": device_ms(lambda: tree.render(starts, directions),
                                                    repeats),
            "first_hit_render_image_wall_ms": wall(lambda: tree.render_image(sampler, 0),
                                                   repeats)[0]}


def rig(num_cameras, size):
    """The cameras of make_mesh_npz.py, in its shuffled order."""
    from bench import synthetic_rig
    intr, poses = synthetic_rig(num_cameras, size)
    cameras = [ffn.CameraInfo.create("c%03d" % i, ffn.Resolution(size, size), intr, p)
               for i, p in enumerate(poses)]
    order = torch.randperm(num_cameras, generator=torch.Generator().manual_seed(0)).numpy()
    return [cameras[i] for i in order]


def mesh_frames(points, triangles, uvs, texture, cameras, supersample):
    size = cameras[0].resolution.width
    images = np.zeros((len(cameras), size, size, 4), np.uint8)
    for index, camera in enumerate(cameras):
        color, alpha, _ = ffn.render_mesh_image(points, triangles, camera, uvs=uvs, texture=texture,
                                                include_depth=True, supersample=supersample)
        images[index, ..., :3] = color
        images[index, ..., 3] = np.rint(255 * alpha)
    return images


def voxel_frames(truth, cameras, bounds):
    size = cameras[0].resolution.width
    sampler = quiet(ffn.RaySampler, bounds, cameras, 8)
    images = np.zeros((len(cameras), size, size, 4), np.uint8)
    for index in range(len(cameras)):
        color, alpha, _ = truth.render_image(sampler, index, shading="flat", include_depth=True)
        images[index, ..., :3] = color
        images[index, ..., 3] = np.where(alpha > 0, 255, 0)
    return images


def psnr_of_mesh(surface, held):
    """Colour PSNR of a SurfaceMesh drawn by K31 over every pixel of the held-out cameras."""
    sampler = held.sampler
    per = sampler.rays_per_camera
    v, t, c = (on_gpu(surface.vertices, "float32"), on_gpu(surface.triangles, "int32"),
               on_gpu(surface.colors, "float32"))
    error = 0.0
    for index, camera in enumerate(sampler.cameras):
        out, _ = ffn.render_mesh(v, t, camera, colors=c)
        truth = held.colors[index * per:(index + 1) * per]
        error += float(((out.color - truth) ** 2).sum(dtype=torch.float64).item())
    return float(-10 * np.log10(max(error / (3 * per * sampler.num_cameras), 1e-12)))


def quality(args, results, write):
    torus = ffn.procedural_torus()
    vertices, triangles, uvs, texture = torus
    points = ffn.normalize_points(vertices)
    cameras = rig(args.cameras, args.size)
    bounds = np.diag([2, 2, 2, 1]).astype(np.float32)
    truth = ffn.OcTree.build_from_triangles(*torus, args.truth_depth, 4)
    center, scale = truth.center, truth.scale
    k22 = ffn.OcTree.build_from_triangles(*torus, args.fit_depth, 4)
    train_n = args.cameras - HELD_OUT
    experiment = {"depth": args.fit_depth, "train_cameras": train_n, "held_out_cameras": HELD_OUT,
                  "fit_steps": FIT_STEPS, "frames": [args.size, args.size], "ground_truths": {}}
    results["held_out_psnr"] = experiment
    sources = [("voxel_depth_%d" % args.truth_depth, lambda: voxel_frames(truth, cameras, bounds))]
    for k in args.supersamples:
        sources.append(("mesh_supersample_%d" % k,
                        lambda k=k: mesh_frames(points, triangles, uvs, texture, cameras, k)))
    for name, make in sources:
        images = make()
        train = quiet(ffn.ImageDataset, "train", images[:train_n], bounds, cameras[:train_n], 8,
                      device="cuda")
        held = quiet(ffn.ImageDataset, "val", images[train_n:], bounds, cameras[train_n:], 8,
                     device="cuda")
        entry = {"hit_share": float((images[..., 3] > 0).mean())}
        experiment["ground_truths"][name] = entry
        carved = ffn.OcTree.build_from_silhouettes(train, args.fit_depth, center, scale)
        entry["carved_leaves"] = carved.num_leaves
        entry["psnr_carved_as_built"] = psnr_all_pixels(
            lambda s, d: carved.render_volume(s, d).color, held, center)
        fitted, log = ffn.fit_octree(carved, train, None, num_steps=FIT_STEPS, verbose=False)
        entry["psnr_after_fit_octree"] = psnr_all_pixels(
            lambda s, d: fitted.render_volume(s, d).color, held, center)
        entry["psnr_k22_depth_%d_tree_first_hit" % args.fit_depth] = psnr_all_pixels(
            lambda s, d: k22.render(s, d).color, held, k22.center)
        write()
        for placement in ("corners", "surface_nets"):
            surface = fitted.extract_mesh(placement=placement, center=center)
            entry["fitted_mesh_%s" % placement] = {
                "triangles": len(surface.triangles), "psnr_drawn_by_k31": psnr_of_mesh(surface, held)}
        print(json.dumps({name: entry}), flush=True)
        write()
        del train, held, carved, fitted
        torch.cuda.empty_cache()


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--repeats", type=int, default=5)
    parser.add_argument("--depths", type=int, nargs="*", default=[8, 10])
    parser.add_argument("--size", type=int, default=400)
    parser.add_argument("--cameras", type=int, default=120)
    parser.add_argument("--truth-depth", type=int, default=9)
    parser.add_argument("--fit-depth", type=int, default=8)
    parser.add_argument("--supersamples", type=int, nargs="*", default=[1, 4])
    parser.add_argument("--skip-quality", action="store_true")
    parser.add_argument("--out", default=DEFAULT_OUT)
    args = parser.parse_args()
    results = {"device": torch.cuda.get_device_name(0), "frame": [args.size, args.size],
               "repeats": args.repeats, "precision": "f32 and integers (no matrix work on this path)",
               "rocprofv3_kernel_times": "not collected", "cases": [], "complete": False}

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(results, indent=1) + "\n")

    camera = rig(8, args.size)[0]
    bounds = np.diag([2, 2, 2, 1]).astype(np.float32)
    sampler = quiet(ffn.RaySampler, bounds, [camera], 8, device="cuda")
    torus = ffn.procedural_torus()
    case = {"mesh": "procedural_torus(), normalised, textured"}
    case.update(raster_case(ffn.normalize_points(torus[0]), torus[1], camera, args.repeats,
                            uvs=torus[2], texture=torus[3]))
    case["tree"] = first_hit_case(ffn.OcTree.build_from_triangles(*torus, args.fit_depth, 4),
                                  sampler, args.repeats)
    results["cases"].append(case)
    print(json.dumps(case), flush=True)
    write()
    model = opaque_ball() if args.depths else None
    for depth in args.depths:
        tree = ffn.OcTree.build_from_model(model, depth, alpha_threshold=0.01)
        surface = tree.extract_mesh(0.01)
        case = {"mesh": "extract_mesh(0.01, surface_nets) of the depth-%d density tree" % depth}
        case.update(raster_case(surface.vertices, surface.triangles, camera, args.repeats,
                                colors=surface.colors))
        case["tree"] = first_hit_case(tree, sampler, args.repeats)
        results["cases"].append(case)
        print(json.dumps(case), flush=True)
        write()
        del tree, surface
        torch.cuda.empty_cache()
    if not args.skip_quality:
        quality(args, results, write)
    results["complete"] = True
    write()
    return 0


if __name__ == "__main__":
    sys.exit(main())
