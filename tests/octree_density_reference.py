"""Numpy restatement of the K16 density-octree build (``OcTree.build_from_model``), sharing no code
with the package: the f32 centre chain of a finest cell, the occupancy rule, the bottom-up merge
passes and the node ids.

Everything that the kernels round in f32 is rounded in f32 here, operation by operation.  The
activations are the exception: ``activate`` is numpy's exp in f32, which need not agree with the
device's to the last bit, so a test that compares bits passes the device's own activations
(``ops.octree_bake`` of the same logits) as ``data``."""

import numpy as np

F = np.float32


def first_id(level):
    """Id of the first node of ``level``: (8^level - 1) / 7."""
    return (8 ** int(level) - 1) // 7


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


def activate(logits):
    """[sigmoid(r), sigmoid(g), sigmoid(b), softplus(sigma)] in f32 numpy (beta 1, threshold 20)."""
    x = np.asarray(logits, F)
    with np.errstate(over="ignore"):
        rgb = (F(1) / (F(1) + np.exp(-x[:, :3]))).astype(F)
        soft = np.where(x[:, 3] > F(20), x[:, 3], np.log1p(np.exp(np.minimum(x[:, 3], F(20)))))
    return np.concatenate([rgb, soft.astype(F)[:, None]], 1).astype(F)


def tau_of(alpha_threshold):
    return F(-np.log1p(-np.float64(alpha_threshold)))


def side_of(scale, depth):
    return F(F(2) * F(scale) / F(2.0 ** (depth - 1)))


def select(data, first_code, tau, side):
    """data (N,4) f32, activated -> (codes int32, data) of the rows with sigma * side > tau."""
    data = np.asarray(data, F)
    with np.errstate(invalid="ignore", over="ignore"):
        keep = (data[:, 3] * F(side)).astype(F) > F(tau)          # NaN: False
    codes = (first_code + np.nonzero(keep)[0]).astype(np.int32)
    return codes, data[keep]


def merge_level(codes, levels, data, level, depth, rgb_tol, sigma_tol):
    """One pass: eight consecutive entries, all leaves of ``level``, children 0 .. 7 of one parent,
    every channel within the tolerance of the mean -> the parent."""
    codes, levels, data = np.asarray(codes, np.int32), np.asarray(levels, np.int32), np.asarray(data, F)
    n = len(codes)
    shift = 3 * (depth - 1 - level)
    digit = (codes.astype(np.int64) >> shift) & 7
    heads = np.nonzero((levels == level) & (digit == 0))[0]
    heads = heads[heads + 7 < n]
    span = heads[:, None] + np.arange(8)[None, :]
    if len(heads):
        same = (levels[span] == level).all(1)
        same &= (codes[heads + 7].astype(np.int64) >> shift) == (codes[heads].astype(np.int64) >> shift) + 7
        heads, span = heads[same], span[same]
    group = data[span]                                            # (G,8,4)
    total = group[:, 0].copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(1, 8):
            total = (total + group[:, k]).astype(F)
        mean = (total * F(0.125)).astype(F)
        off = np.abs((group - mean[:, None, :]).astype(F))
        tol = np.array([rgb_tol, rgb_tol, rgb_tol, sigma_tol], F)
        ok = (off <= tol[None, None, :]).all((1, 2))              # NaN: False
    heads, mean = heads[ok], mean[ok]
    keep = np.ones(n, bool)
    for k in range(1, 8):
        keep[heads + k] = False
    levels, data = levels.copy(), data.copy()
    levels[heads] = level - 1
    data[heads] = mean
    return codes[keep], levels[keep], data[keep]


def merge(codes, levels, data, depth, rgb_tol, sigma_tol, passes=None):
    """Level depth-1 down to level 1; ``passes``: a list that receives the state after each."""
    for level in range(depth - 1, 0, -1):
        codes, levels, data = merge_level(codes, levels, data, level, depth, rgb_tol, sigma_tol)
        if passes is not None:
            passes.append((codes, levels, data))
    return codes, levels, data


def leaf_ids(codes, levels, depth):
    codes, levels = np.asarray(codes, np.int64), np.asarray(levels, np.int64)
    base = np.array([first_id(k) for k in range(depth)], np.int64)
    return base[levels] + (codes >> (3 * (depth - 1 - levels)))


def tree(codes, levels, data, depth):
    """-> node_index, leaf_index (sorted int64) and leaf_data in leaf_index order."""
    ids = leaf_ids(codes, levels, depth)
    order = np.argsort(ids, kind="stable")
    nodes = set()
    up = np.unique(ids)
    while len(up) and up.max() > 0:
        up = np.unique((up[up > 0] - 1) >> 3)
        nodes.update(up.tolist())
    node_index = np.array(sorted(nodes - set(ids.tolist())), np.int64)
    return node_index, ids[order], np.asarray(data, F)[order]


def build(logits_or_data, depth, scale, alpha_threshold, merge_tolerance=None, activated=True):
    """The whole build from the values of all 8^(depth-1) cells in code order."""
    data = np.asarray(logits_or_data, F) if activated else activate(logits_or_data)
    codes, data = select(data, 0, tau_of(alpha_threshold), side_of(scale, depth))
    levels = np.full(len(codes), depth - 1, np.int32)
    if merge_tolerance is not None:
        codes, levels, data = merge(codes, levels, data, depth, *merge_tolerance)
    return tree(codes, levels, data, depth)
