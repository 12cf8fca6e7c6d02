"""Numpy restatement of K28 (``csrc/octree_walk.hip`` mode kVisibleMoments,
``ops.octree_visible_moments``, ``photo_actions``, ``OcTree.carve_photo``), sharing no code with the
package.

* The moments are the ``visible`` matrix of ``tests/visible_reference.visible`` -- which (leaf,
  camera) pairs are decided visible -- summed into sums, counts and squares of the bytes the pairs
  project to (``visible_reference.project``).  Its undecided pairs are reported, not summed.
* The policy is restated in Python integers of unbounded size: ``n Q - S > limit n^2`` with
  ``limit = ceil(3 (255 threshold)^2)``.
* The sweep loop is restated on sets of leaf ids: a tree is its sorted leaf ids and the set of
  their ancestors.
"""

import math

import numpy as np

from tests import visible_reference as vref

F = np.float32
DROP, KEEP = 0, 1


def moments(scale, node_index, leaf_index, density, images, proj, eyes, alpha_u8, tau):
    """-> dict: ``moments`` (L,8) int64 ``[sum_r, sum_g, sum_b, count, sq_r, sq_g, sq_b, 0]`` over
    the pairs decided visible, ``visible`` / ``undecided`` / ``candidate`` (L,C) bool, ``pairs``."""
    got = vref.visible(scale, node_index, leaf_index, density, images, proj, eyes, alpha_u8, tau)
    images = np.asarray(images, np.uint8)
    cameras, height, width = images.shape[:3]
    centers = vref.centers_of(scale, leaf_index)
    out = np.zeros((len(leaf_index), 8), np.int64)
    for c in range(cameras):
        _, col, row = vref.project(centers, np.asarray(proj, F)[c], width, height)
        rgb = images[c, row, col, :3].astype(np.int64)
        sees = got["visible"][:, c]
        out[sees, :3] += rgb[sees]
        out[sees, 3] += 1
        out[sees, 4:7] += rgb[sees] ** 2
    assert np.array_equal(out[:, :4], got["votes"])
    return dict(moments=out, visible=got["visible"], undecided=got["undecided"],
                candidate=got["candidate"], pairs=got["pairs"])


def limit_of(threshold):
    return int(math.ceil(3.0 * (255.0 * float(threshold)) ** 2))


def actions(moments_, threshold, min_views=2):
    """(L,) uint8 of DROP / KEEP, in Python integers."""
    limit = limit_of(threshold)
    out = np.full(len(moments_), KEEP, np.uint8)
    for k, row in enumerate(np.asarray(moments_).tolist()):
        n, spread = row[3], row[4] + row[5] + row[6]
        squares = row[0] ** 2 + row[1] ** 2 + row[2] ** 2
        if n >= min_views and n * spread - squares > limit * n * n:
            out[k] = DROP
    return out


def variance(moments_):
    """float64 (L,): the mean over the channels of the per-channel variance of the seeing
    cameras' pixels, colours in [0, 1]; NaN where no camera sees."""
    m = np.asarray(moments_, np.float64)
    with np.errstate(all="ignore"):
        mean = m[:, :3] / m[:, 3:4]
        return ((m[:, 4:7] / m[:, 3:4] - mean ** 2) / 255.0 ** 2).mean(1)


def tree_of(leaf_ids):
    """The tree whose leaves are ``leaf_ids``: -> node_index (their ancestors), leaf_index, both
    sorted int64."""
    nodes = set()
    for node in np.asarray(leaf_ids, np.int64).tolist():
        while node > 0:
            node = (node - 1) // 8
            nodes.add(node)
    return np.array(sorted(nodes), np.int64), np.array(sorted(leaf_ids), np.int64)


def carve(scale, leaf_index, density_of, images, proj, eyes, alpha_u8, tau, threshold,
          min_views=2, max_sweeps=16):
    """The loop of ``carve_photo`` on leaf ids.  ``density_of``: dict id -> density.  -> dict:
    ``leaf_index`` of the final tree, ``converged``, ``sweeps``: per sweep a dict with the
    ``leaf_index`` before it, its ``moments``, ``seen``, ``judged``, the ``dropped`` ids and the
    number of ``undecided`` pairs."""
    ids = np.array(sorted(np.asarray(leaf_index, np.int64).tolist()), np.int64)
    sweeps, converged = [], False
    for _ in range(max_sweeps):
        nodes, ids = tree_of(ids)
        density = np.array([density_of[int(i)] for i in ids], F)
        got = moments(scale, nodes, ids, density, images, proj, eyes, alpha_u8, tau)
        action = actions(got["moments"], threshold, min_views)
        count = got["moments"][:, 3]
        dropped = ids[action == DROP]
        sweeps.append(dict(leaf_index=ids, moments=got["moments"], seen=int((count > 0).sum()),
                           judged=int((count >= min_views).sum()), dropped=dropped,
                           undecided=int(got["undecided"].sum())))
        if len(dropped) == 0:
            converged = True
            break
        assert len(dropped) < len(ids), "the sweep would drop every leaf"
        ids = ids[action != DROP]
    return dict(leaf_index=ids, converged=converged, sweeps=sweeps)


def colors(moments_, before):
    """``visible_reference.colors`` of the first four fields."""
    return vref.colors(np.asarray(moments_)[:, :4], before)
