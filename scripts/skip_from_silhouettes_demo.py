"""Empty-space skipping from step 0 with nothing but the dataset (DESIGN K25): the protocol of
scripts/skip_training_demo.py -- its scene, seeds, step count and PSNR function, by import -- with
the arms (A) full steps, (B) the analytic sphere grid from step 0, (D) the grid that
``OccupancyGrid.from_silhouettes(train, resolution=128, depth=8)`` carves from the training
images, defaults throughout, from step 0.  Per arm: ms per step, mean evaluated fraction, held-out
PSNR under the full render and under the arm's own grid; for D also its build time and the share
of B's bits it lacks -- what the hull lost.  The claim to confirm or refute: D is as fast as B and
within noise of B's PSNR under its own grid.  Recorded as it comes out, nothing tuned afterwards.

    python scripts/skip_from_silhouettes_demo.py [--steps 1200] [--out result.json]
"""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import fourier_feature_nets_amd as ffn  # noqa: E402
import skip_training_demo as protocol  # noqa: E402

DEFAULT_OUT = os.path.join(ROOT, "profiles", "r23_skip_from_silhouettes_demo.json")


def bit_count(bits):
    words = bits.to(torch.int64) & 0xffffffff
    return sum(int(((words >> shift) & 1).sum().item()) for shift in range(32))


def main():
    argv = sys.argv[1:]
    out_path = DEFAULT_OUT
    if "--out" in argv:
        at = argv.index("--out")
        out_path = argv[at + 1]
        del argv[at:at + 2]
    args = protocol.parse_args(argv)
    dev = torch.device("cuda:0")
    scene = protocol.make_scene(args, dev)

    ffn.OccupancyGrid.from_silhouettes(scene.train, resolution=128, depth=8)      # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    hull = ffn.OccupancyGrid.from_silhouettes(scene.train, resolution=128, depth=8)
    torch.cuda.synchronize()
    build_ms = 1e3 * (time.perf_counter() - t0)

    runs = {"A_full": protocol.run_arm(scene, args, dev),
            "B_analytic_grid": protocol.run_arm(scene, args, dev, grid=scene.analytic),
            "D_silhouette_grid": protocol.run_arm(scene, args, dev, grid=hull)}
    b_bits, d_bits = scene.analytic.bits, hull.bits
    lacking = bit_count(b_bits & ~d_bits)
    runs["D_silhouette_grid"].update({
        "from_silhouettes_wall_ms": round(build_ms, 2),
        "fraction_occupied": round(hull.fraction_occupied(), 5),
        "bits": bit_count(d_bits),
        "bits_of_B_that_D_lacks": lacking,
        "share_of_B_bits_that_D_lacks": round(lacking / max(bit_count(b_bits), 1), 6)})
    runs["B_analytic_grid"].update({"fraction_occupied": round(scene.analytic.fraction_occupied(), 5),
                                    "bits": bit_count(b_bits)})
    b, d = runs["B_analytic_grid"], runs["D_silhouette_grid"]
    out = {"device": torch.cuda.get_device_name(0),
           "scene": protocol.scene_line(scene, args),
           "note": "A = reference-exact step; B = the analytic sphere grid of skip_training_demo.py "
                   "from step 0; D = OccupancyGrid.from_silhouettes(train, resolution=128, depth=8) "
                   "from step 0, defaults (carve: alpha_threshold 0.5, dilate 1, max_misses 0, "
                   "min_views 2; grid: dilate 1).  Same weights, same batches.  A model trained "
                   "under a grid from step 0 is judged under that grid.",
           "claim": "D is as fast as B and within noise of B's PSNR under its own grid",
           "D_over_B_ms_per_step": round(d["ms_per_step"] / b["ms_per_step"], 4),
           "D_minus_B_psnr_db_under_own_grid": round(d["val_psnr_db_rendered_with_its_grid"]
                                                     - b["val_psnr_db_rendered_with_its_grid"], 3),
           "not_measured": "rocprofv3 kernel times; --precision bf16x6; seeds other than the protocol's",
           "runs": runs}
    line = json.dumps(out, indent=1)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
