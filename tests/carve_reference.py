"""Numpy restatement of K23 (``csrc/carve.hip``, ``ops.octree_carve_select``), sharing no code with
the package: the f32 centre chain of a finest cell, the projection with every product and sum
rounded on its own, the nearest pixel, the votes as integers, the keep rule and the colour.

The cameras are looped over in order and every step is a whole-array f32 operation, so that numpy
rounds where the kernel rounds.  ``early_out=True`` drops a cell from the loop once it has more
than ``max_misses`` misses, as the kernel does; ``early_out=False`` visits every camera for every
cell and decides at the end.  The kept cells and their rows are the same either way (the tests
check it); only ``visited`` differs."""

import numpy as np

F = np.float32


def cell_centers(first_code, count, center, scale, depth):
    """(count,3) f32: the chain +-scale/2^k from 0 along the digits of the code, root first, then
    one f32 add of the cube's centre."""
    codes = np.arange(first_code, first_code + count, dtype=np.int64)
    c = np.zeros((count, 3), F)
    half = F(scale)
    for level in range(1, depth):
        half = F(half * F(0.5))
        digit = (codes >> (3 * (depth - 1 - level))) & 7
        for axis, bit in enumerate((4, 2, 1)):
            c[:, axis] = np.where(digit & bit, c[:, axis] + half, c[:, axis] - half).astype(F)
    return (c + np.asarray(center, F)[None, :]).astype(F)


def project(points, matrix, width, height):
    """points (N,3) f32, matrix (3,4) f32 -> seen (N) bool, col (N), row (N) int64 (0 where not
    seen).  x = ((P00 px + P01 py) + P02 pz) + P03 and so on; !(w > 0) is not seen; fu = x / w +
    0.5; seen iff 0 <= fu < W and 0 <= fv < H; col = (int)fu."""
    p = np.asarray(points, F)
    m = np.asarray(matrix, F)
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        def line(r):
            return (((m[r, 0] * px).astype(F) + (m[r, 1] * py).astype(F)).astype(F)
                    + (m[r, 2] * pz).astype(F)).astype(F) + m[r, 3]
        x, y, w = line(0).astype(F), line(1).astype(F), line(2).astype(F)
        front = w > F(0)                                           # NaN: False
        safe = np.where(front, w, F(1))
        fu = ((x / safe).astype(F) + F(0.5)).astype(F)
        fv = ((y / safe).astype(F) + F(0.5)).astype(F)
        seen = front & (fu >= F(0)) & (fu < F(width)) & (fv >= F(0)) & (fv < F(height))
    col = np.where(seen, fu, F(0)).astype(np.int64)                # truncation, values >= 0
    row = np.where(seen, fv, F(0)).astype(np.int64)
    return seen, col, row


def carve(images, mask, proj, first_code, count, center, scale, depth, alpha_u8, max_misses,
          min_views, sigma0, early_out=True):
    """images (C,H,W,4) u8, mask (C,H,W) u8, proj (C,3,4) f32 -> codes (K) int32, data (K,4) f32 of
    the kept cells in code order, and visited (count) int32: the cameras each cell's loop looked
    at."""
    images, mask = np.asarray(images, np.uint8), np.asarray(mask, np.uint8)
    cameras, height, width = mask.shape
    points = cell_centers(first_code, count, center, scale, depth)
    seen_n = np.zeros(count, np.int64)
    misses = np.zeros(count, np.int64)
    colored = np.zeros(count, np.int64)
    sums = np.zeros((count, 3), np.int64)
    visited = np.zeros(count, np.int32)
    alive = np.ones(count, bool)
    for c in range(cameras):
        live = np.nonzero(alive)[0] if early_out else np.arange(count)
        if len(live) == 0:
            break
        visited[live] += 1
        seen, col, row = project(points[live], proj[c], width, height)
        live, col, row = live[seen], col[seen], row[seen]
        seen_n[live] += 1
        hit = mask[c, row, col] != 0
        misses[live[~hit]] += 1
        if early_out:
            alive[live[~hit]] = misses[live[~hit]] <= max_misses
        live, col, row = live[hit], col[hit], row[hit]
        rgba = images[c, row, col]
        own = rgba[:, 3] >= alpha_u8
        sums[live[own]] += rgba[own, :3].astype(np.int64)
        colored[live[own]] += 1
    keep = (misses <= max_misses) & (seen_n >= min_views)
    data = np.full((count, 4), F(0.5), F)
    data[:, 3] = F(sigma0)
    some = colored > 0
    assert (255 * colored).max(initial=0) <= 2 ** 24
    denominator = (255 * colored[some]).astype(F)
    for ch in range(3):
        data[some, ch] = (sums[some, ch].astype(F) / denominator).astype(F)
    codes = (first_code + np.nonzero(keep)[0]).astype(np.int32)
    return codes, data[keep], visited


def grow(mask, dilate):
    """(C,H,W) 0/1 mask grown by ``dilate`` pixels: the maximum over the (2 dilate + 1)^2 square."""
    mask = np.asarray(mask, np.uint8)
    if dilate == 0:
        return mask.copy()
    cameras, height, width = mask.shape
    padded = np.zeros((cameras, height + 2 * dilate, width + 2 * dilate), np.uint8)
    padded[:, dilate:dilate + height, dilate:dilate + width] = mask
    out = np.zeros_like(mask)
    for dy in range(2 * dilate + 1):
        for dx in range(2 * dilate + 1):
            out = np.maximum(out, padded[:, dy:dy + height, dx:dx + width])
    return out
