"""Numpy restatement of K27 (``csrc/carve_box.hip``, ``ops.octree_carve_box_level``), sharing no
code with the package: the conservative, coarse-to-fine space carve.  A cell of level k is a centre
and eight corners; a camera refutes the cell only when all nine are in front of it and the padded
bounding rectangle of their pixels lies inside the image and holds no foreground pixel.

Every step is a whole-array f32 operation, so that numpy rounds where the kernel rounds; the
summed-area table holds integers.  ``box_level`` tests a list of cells of one level, ``box_carve``
runs coarse to fine from a start level, ``box_flat`` tests every finest cell."""

import numpy as np

from tests import carve_reference as cref

F = np.float32
LIMIT = F(2.0 ** 30)
SIGNS = [(sx, sy, sz) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]     # x slowest


def tables(mask):
    """(C,H,W) mask -> (C,H+1,W+1) int64: entry [c, r, q] counts the foreground pixels of camera c
    in rows < r and columns < q."""
    mask = (np.asarray(mask) != 0).astype(np.int64)
    cameras, height, width = mask.shape
    sat = np.zeros((cameras, height + 1, width + 1), np.int64)
    sat[:, 1:, 1:] = mask.cumsum(1).cumsum(2)
    return sat


def cell_points(codes, level, center, scale):
    """codes (N) of level ``level`` -> (N,9,3) f32: the centre by the chain +-scale / 2^k along the
    code's digits, root first, plus the cube's centre; then the corners centre -+ half, half being
    scale halved ``level`` times."""
    codes = np.asarray(codes, np.int64)
    c = np.zeros((len(codes), 3), F)
    half = F(scale)
    for step in range(1, level + 1):
        half = F(half * F(0.5))
        digit = (codes >> (3 * (level - step))) & 7
        for axis, bit in enumerate((4, 2, 1)):
            c[:, axis] = np.where(digit & bit, c[:, axis] + half, c[:, axis] - half).astype(F)
    q0 = (c + np.asarray(center, F)[None, :]).astype(F)
    points = np.empty((len(codes), 9, 3), F)
    points[:, 0] = q0
    for k, signs in enumerate(SIGNS):
        for axis in range(3):
            points[:, 1 + k, axis] = (q0[:, axis] + half if signs[axis] > 0
                                      else q0[:, axis] - half).astype(F)
    return points


def footprint(points, matrix, table, width, height, pad):
    """points (N,9,3) f32, one camera's matrix (3,4) and table (H+1,W+1) -> a dict of (N) arrays:
    front (how many points are in front), undecided, c0, c1, r0, r1 (the padded rectangle; only
    meaningful where some point in front has finite pixel coordinates), inside, count (foreground
    pixels in the rectangle where inside, else -1), miss, seen."""
    m = np.asarray(matrix, F)
    px, py, pz = points[..., 0], points[..., 1], points[..., 2]
    with np.errstate(all="ignore"):
        def line(r):
            return ((((m[r, 0] * px).astype(F) + (m[r, 1] * py).astype(F)).astype(F)
                     + (m[r, 2] * pz).astype(F)).astype(F) + m[r, 3]).astype(F)
        x, y, w = line(0), line(1), line(2)
        front = w > F(0)                                             # NaN: False
        safe = np.where(front, w, F(1))
        fu = ((x / safe).astype(F) + F(0.5)).astype(F)
        fv = ((y / safe).astype(F) + F(0.5)).astype(F)
        finite = np.isfinite(fu) & np.isfinite(fv)
        col = np.floor(np.clip(np.where(finite, fu, F(0)), -LIMIT, LIMIT)).astype(np.int64)
        row = np.floor(np.clip(np.where(finite, fv, F(0)), -LIMIT, LIMIT)).astype(np.int64)
    undecided = (front & ~finite).any(1)
    valid = front & finite
    big = np.int64(2) ** 40
    c0 = np.where(valid, col, big).min(1) - pad
    c1 = np.where(valid, col, -big).max(1) + pad
    r0 = np.where(valid, row, big).min(1) - pad
    r1 = np.where(valid, row, -big).max(1) + pad
    count_front = front.sum(1)
    whole = (count_front == 9) & ~undecided
    inside = whole & (c0 >= 0) & (c1 <= width - 1) & (r0 >= 0) & (r1 <= height - 1)
    meets = (c1 >= 0) & (c0 <= width - 1) & (r1 >= 0) & (r0 <= height - 1)
    seen = (count_front > 0) & (undecided | (count_front < 9) | meets)
    a0, a1 = np.where(inside, r0, 0), np.where(inside, r1, 0) + 1
    b0, b1 = np.where(inside, c0, 0), np.where(inside, c1, 0) + 1
    count = table[a1, b1] - table[a0, b1] - table[a1, b0] + table[a0, b0]
    count = np.where(inside, count, -1)
    return dict(front=count_front, undecided=undecided, c0=c0, c1=c1, r0=r0, r1=r1, inside=inside,
                count=count, miss=inside & (count == 0), seen=seen)


def box_level(images, mask, proj, codes, level, center, scale, depth, alpha_u8, max_misses,
              min_views, sigma0, early_out=True, details=None):
    """images (C,H,W,4) u8, mask (C,H,W) u8 (grown), proj (C,3,4) f32, codes (N) of level ``level``
    -> keep (N) bool, data (N,4) f32 (meaningful where keep, at the finest level), visited (N)
    int32.  ``details``, a list, receives each camera's ``footprint`` dict (use early_out=False to
    have every cell in every one of them)."""
    images, mask = np.asarray(images, np.uint8), np.asarray(mask, np.uint8)
    cameras, height, width = mask.shape
    sat = tables(mask)
    codes = np.asarray(codes, np.int64)
    n = len(codes)
    points = cell_points(codes, level, center, scale)
    pad = 1 + (depth - 1 - level)
    finest = level == depth - 1
    seen_n, misses = np.zeros(n, np.int64), np.zeros(n, np.int64)
    colored, sums = np.zeros(n, np.int64), np.zeros((n, 3), np.int64)
    visited = np.zeros(n, np.int32)
    alive = np.ones(n, bool)
    for c in range(cameras):
        live = np.nonzero(alive)[0] if early_out else np.arange(n)
        if len(live) == 0:
            break
        visited[live] += 1
        f = footprint(points[live], proj[c], sat[c], width, height, pad)
        if details is not None:
            details.append(f)
        seen_n[live[f["seen"]]] += 1
        misses[live[f["miss"]]] += 1
        if early_out:
            alive[live] = misses[live] <= max_misses
        if not finest:
            continue
        on, col, row = cref.project(points[live, 0], proj[c], width, height)
        live, col, row = live[on], col[on], row[on]
        rgba = images[c, row, col]
        own = rgba[:, 3] >= alpha_u8
        sums[live[own]] += rgba[own, :3].astype(np.int64)
        colored[live[own]] += 1
    keep = misses <= max_misses
    if finest:
        keep &= seen_n >= min_views
    data = np.full((n, 4), F(0.5), F)
    data[:, 3] = F(sigma0)
    some = colored > 0
    denominator = (255 * colored[some]).astype(F)
    for ch in range(3):
        data[some, ch] = (sums[some, ch].astype(F) / denominator).astype(F)
    return keep, data, visited


def box_carve(images, mask, proj, center, scale, depth, alpha_u8, max_misses, min_views, sigma0,
              start_level, visits=None):
    """Coarse to fine from every cell of ``min(start_level, depth - 1)`` -> codes (K) int32 and data
    (K,4) f32 of the kept finest cells in code order.  ``visits``, a list, gets the number of
    candidates of each level."""
    level = min(start_level, depth - 1)
    codes = np.arange(8 ** level, dtype=np.int64)
    while True:
        if visits is not None:
            visits.append(len(codes))
        keep, data, _ = box_level(images, mask, proj, codes, level, center, scale, depth, alpha_u8,
                                  max_misses, min_views, sigma0)
        codes, data = codes[keep], data[keep]
        if level == depth - 1 or len(codes) == 0:
            return codes.astype(np.int32), data
        codes = ((codes[:, None] << 3) | np.arange(8, dtype=np.int64)[None, :]).reshape(-1)
        level += 1


def box_flat(images, mask, proj, center, scale, depth, alpha_u8, max_misses, min_views, sigma0):
    """Every finest cell tested on its own."""
    codes = np.arange(8 ** (depth - 1), dtype=np.int64)
    keep, data, _ = box_level(images, mask, proj, codes, depth - 1, center, scale, depth, alpha_u8,
                              max_misses, min_views, sigma0)
    return codes[keep].astype(np.int32), data[keep]
