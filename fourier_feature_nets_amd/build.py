"""Builds libffn_hip.so (gfx950) in-tree with hipcc.  No CMake, no JIT cache.

    python -m fourier_feature_nets_amd.build [--force]

The shared library lands next to this file so that it travels with the source tree.
"""

import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
INCLUDE = os.path.join(os.path.dirname(HERE), "include")
LIB_PATH = os.path.join(HERE, "libffn_hip.so")

# name -> extra flags.  The sampling kernels must not contract a*b+c into an FMA: the
# reference's ATen ops round every multiply and add separately.
SOURCES = {
    "abi.hip": [],
    "rays.hip": ["-ffp-contract=off"],
    # (focus.hip: the op-by-op rounding is switched on per function in focus_terms.h -- a
    # file-wide -ffp-contract=off would also change how the math library's own code is compiled,
    # and the fused coarse-pass kernel in mlp.hip has to produce the same bits)
    "focus.hip": [],
    "composite.hip": [],
    "encode.hip": [],
    "optim.hip": ["-ffp-contract=off"],
    "mlp.hip": [],
    "mlp_bf16.hip": [],
    "mlp_bf16_bwd.hip": [],
    # (two waves per SIMD: packed-f32 VALU instructions collide with the other wave's matrix
    # instructions -- keep the compiler from re-packing the unpacked feature / split arithmetic)
    "mlp_bf16_ws.hip": ["-fno-slp-vectorize"],
    "mlp_bf16_mv.hip": ["-fno-slp-vectorize"],
    "wgrad.hip": [],
    "wgrad_bf16.hip": [],
    "wgrad_bf16x6.hip": [],
    "occupancy.hip": [],
    "voxels.hip": [],
    "regression.hip": [],
    # numpy rounds the product and the sum of start + direction * depth separately
    "octree.hip": ["-ffp-contract=off"],
    # plane crossings (plane - o) / d on the f32 chain of node centres, every operation rounded
    "octree_walk.hip": ["-ffp-contract=off"],
    # sums of stored entries in a fixed order: plain adds.  K17b-5 turns a sum of -0 into +0 by
    # adding 0.0f, which -ffast-math or -fno-signed-zeros would fold away: never add those here
    "octree_grad.hip": ["-ffp-contract=off"],
    # d = a - b, s = sqrt(fma(d, d, eps^2)), (s - eps) * scale, (d / s) * scale: only the written
    # fma; tv_finish's + 0.0f is K17b-5's (no -ffast-math here either)
    "octree_tv.hip": ["-ffp-contract=off"],
    # numpy rounds every product and sum of the barycentric and bilinear interpolation separately
    "mesh.hip": ["-ffp-contract=off"],
    # the projection x = ((P00 px + P01 py) + P02 pz) + P03 rounds every product and sum separately
    "carve.hip": ["-ffp-contract=off"],
    # the same projection on a cell's centre and eight corners, operation for operation
    "carve_box.hip": ["-ffp-contract=off"],
    # position = centre + ((c - n / 2) + offset) * side and the fixed-order sums of the offsets,
    # colours and normals, every operation rounded on its own
    "octree_mesh.hip": ["-ffp-contract=off"],
    # K23's projection, the perspective-correct weights and the interpolation of colours, UVs and
    # positions, every product, sum and quotient rounded on its own
    "mesh_raster.hip": ["-ffp-contract=off"],
    # K31c's b_i = q_i * depth_w and the sums of b_i * g over pixels, every product and add rounded
    "mesh_raster_grad.hip": ["-ffp-contract=off"],
    # K31c's UV interpolation and K22's bilinear weights again, and the sums of w * texel and
    # w * g in a fixed order, every product and add rounded
    "mesh_texture.hip": ["-ffp-contract=off"],
    # the edge crossing alpha = E(a) / (E(a) - E(b)), the blends out + m * (in[s] - in[p]) and the
    # sums of the vertex entries in a fixed order, every product, add and quotient rounded
    "mesh_aa.hip": ["-ffp-contract=off"],
    # lambda_i = E_i / |A|, r_i = (a_i depth_w) / w_i, G = (r0 n0 + r1 n1) + r2 n2 and the sums of
    # -(lambda_j G) over pixels and corners in a fixed order, every operation rounded on its own
    "mesh_interp_grad.hip": ["-ffp-contract=off"],
    # the slab test (lo - o) * inv and Moeller-Trumbore's cross and dot products, K36d's
    # (c0 b0 + c1 b1) + c2 b2: every product, sum and quotient rounded on its own
    "mesh_cast.hip": ["-ffp-contract=off"],
}
COMMON = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", INCLUDE, "-I", CSRC,
          "-Wno-unused-result"]


def _hipcc():
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if cand and (os.path.isabs(cand) and os.path.exists(cand) or not os.path.isabs(cand)):
            return cand
    raise RuntimeError("hipcc not found")


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    stamp = os.path.getmtime(target)
    return any(os.path.getmtime(d) > stamp for d in deps)


def build_library(force=False, verbose=True):
    hipcc = _hipcc()
    headers = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    headers.append(os.path.join(INCLUDE, "ffn_hip.h"))
    obj_dir = os.path.join(CSRC, "build")
    os.makedirs(obj_dir, exist_ok=True)
    jobs, objects = [], []
    for name, extra in SOURCES.items():
        src = os.path.join(CSRC, name)
        if not os.path.exists(src):
            # a kernel file that went missing must fail the BUILD, not surface later as an
            # AttributeError on a symbol the smaller library does not export
            raise RuntimeError("source file listed in SOURCES is missing: %s" % src)
        obj = os.path.join(obj_dir, name.replace(".hip", ".o"))
        objects.append(obj)
        if force or _stale(obj, [src] + headers):
            jobs.append([hipcc] + COMMON + extra + ["-c", src, "-o", obj])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        res = subprocess.run(cmd, capture_output=True, text=True)
        if res.returncode != 0:
            raise RuntimeError("hipcc failed:\n%s\n%s" % (res.stdout, res.stderr))
        if verbose and res.stderr.strip():
            print(res.stderr, file=sys.stderr)

    if jobs:
        with ThreadPoolExecutor(max_workers=min(8, len(jobs))) as pool:
            list(pool.map(run, jobs))
    if jobs or force or _stale(LIB_PATH, objects):
        run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB_PATH] + objects)
    return LIB_PATH


if __name__ == "__main__":
    print(build_library(force="--force" in sys.argv))
