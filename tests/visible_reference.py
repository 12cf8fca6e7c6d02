"""Numpy restatement of K24 (``csrc/octree_walk.hip`` mode kVisible, ``ops.octree_visible_votes``),
sharing no code with the package: which cameras see a leaf through the tree, and the integer sums
of what they see.

* The projection is f32, operation for operation (``project`` below restates
  ``tests/carve_reference.project``: every product and sum rounded on its own, ``!(w > 0)`` not seen,
  ``fu = x / w + 0.5``, the truncated pixel), on the leaves' f32 chain centres
  (``tests/octree_reference.leaf_geometry``), and the ray is ``o = eye``, ``d = centre - eye`` in f32.
* The walk is ``tests/octree_walk_reference.walk``: a float64 enumeration of the regions a ray
  crosses, with no order of visits to get wrong.  Over the crossings of a ray that are leaves with
  ``t_out > 0``, in order of entry: the pair's own leaf makes it VISIBLE; any other leaf multiplies
  the float64 transmittance by ``1 - a``, ``a = 1 - exp(-(max(density, 0) * chord))`` with
  ``chord = (t_out - max(t_in, 0)) |d|``; ``T <= tau`` makes the pair OCCLUDED; a list that ends
  before the pair's own leaf leaves it not visible.
* TWO DEVIATIONS from a plain float64 transmittance with the single criterion ``|T - tau| <= 1e-4
  tau``, both of which can only ADD to what is left out of a comparison and neither of which
  leaves out any pair of the tests' scenes: ``a`` is rounded to f32, and two more criteria make a
  pair undecided (next two items).
* ``a`` is rounded to f32 once (``T`` stays float64).  That rounding is part of the contract, not
  noise: ``1 - expf(-x)`` is exactly 1 in f32 once ``exp(-x) <= 2^-25`` (x > 17.33), which makes
  ``T`` exactly 0 behind a cell that opaque, and with ``tau = 0`` this is the ONLY way a pair is
  occluded -- in exact arithmetic ``T`` never reaches 0.  For ``tau`` well above 2^-24 the rounding
  moves ``T`` by parts in 10^8 and changes nothing.
* A pair is UNDECIDED when, at any step before its decision, ``|T - tau| <= 1e-4 tau`` (f32 against
  float64 may then fall on either side), when ``exp(-x)`` lies within 1e-4 (relative) of 2^-25 (the
  f32 rounding of ``a`` to 1 may then go either way), or when ``0 < T < 1e-30`` (f32 underflow).
  Undecided pairs are left out of comparisons; every test asserts that they are at most 1 % of its
  pairs.  A crossing of zero chord (a sliver that the walk and the enumeration may or may not both
  see) multiplies ``T`` by 1 and makes nothing undecided.
"""

import numpy as np

from tests import octree_reference as oref
from tests import octree_walk_reference as wref

F = np.float32
BAND = 1e-4


def project(points, matrix, width, height):
    """points (N,3) f32, matrix (3,4) f32 -> seen (N) bool, col (N), row (N) int64 (0 where not
    seen)."""
    p = np.asarray(points, F)
    m = np.asarray(matrix, F)
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        def line(r):
            first = ((m[r, 0] * px).astype(F) + (m[r, 1] * py).astype(F)).astype(F)
            return ((first + (m[r, 2] * pz).astype(F)).astype(F) + m[r, 3]).astype(F)
        x, y, w = line(0), line(1), line(2)
        front = w > F(0)                                           # NaN: False
        safe = np.where(front, w, F(1))
        fu = ((x / safe).astype(F) + F(0.5)).astype(F)
        fv = ((y / safe).astype(F) + F(0.5)).astype(F)
        seen = front & (fu >= F(0)) & (fu < F(width)) & (fv >= F(0)) & (fv < F(height))
    col = np.where(seen, fu, F(0)).astype(np.int64)                # truncation, values >= 0
    row = np.where(seen, fv, F(0)).astype(np.int64)
    return seen, col, row


def centers_of(scale, leaf_index):
    """(L,3) f32: the leaves' centres relative to the cube's centre."""
    return oref.leaf_geometry(np.float32(scale), np.asarray(leaf_index, np.int64))[0].astype(F)


def visible(scale, node_index, leaf_index, density, images, proj, eyes, alpha_u8, tau,
            centers=None):
    """density (L,) (any float dtype; read as f32), images (C,H,W,4) u8, proj (C,3,4) f32 for
    cube-relative points, eyes (C,3) f32 -> dict: ``votes`` (L,4) int64 over the pairs decided
    visible, ``candidate`` / ``visible`` / ``undecided`` (L,C) bool (a candidate passed the
    projection and the pixel's alpha; visible and undecided are subsets of it), ``pairs`` = L C."""
    leaf_index = np.asarray(leaf_index, np.int64)
    density = np.asarray(density, F).astype(np.float64)
    images = np.asarray(images, np.uint8)
    proj, eyes = np.asarray(proj, F), np.asarray(eyes, F)
    cameras, height, width = images.shape[:3]
    if centers is None:
        centers = centers_of(scale, leaf_index)
    count = len(leaf_index)
    tau = float(tau)
    candidate = np.zeros((count, cameras), bool)
    seen_it = np.zeros((count, cameras), bool)
    unsure = np.zeros((count, cameras), bool)
    votes = np.zeros((count, 4), np.int64)
    for c in range(cameras):
        ok, col, row = project(centers, proj[c], width, height)
        rgba = images[c, row, col]
        ok &= rgba[:, 3] >= alpha_u8
        candidate[:, c] = ok
        which = np.nonzero(ok)[0]
        if len(which) == 0:
            continue
        starts = np.repeat(eyes[c][None, :], len(which), 0).astype(F)
        directions = (centers[which] - starts).astype(F)
        w = wref.walk(scale, node_index, leaf_index, starts, directions)
        norm = np.linalg.norm(directions.astype(np.float64), axis=1)
        for k, leaf in enumerate(which):
            trans, found, doubt = 1.0, False, False
            for at in range(w["offsets"][k], w["offsets"][k + 1]):
                other = w["leaf"][at]
                if other < 0 or not w["t_out"][at] > 0.0:
                    continue
                if other == leaf:
                    found = True
                    break
                sigma = density[other]
                sigma = sigma if sigma > 0.0 else 0.0               # negative and NaN: 0
                x = sigma * ((w["t_out"][at] - max(w["t_in"][at], 0.0)) * norm[k])
                e = np.exp(-x)
                if abs(e * 2.0 ** 25 - 1.0) <= BAND:
                    doubt = True
                trans *= 1.0 - np.float64(F(1.0 - e))
                if (tau > 0.0 and abs(trans - tau) <= BAND * tau) or 0.0 < trans < 1e-30:
                    doubt = True
                if trans <= tau:
                    break
            unsure[leaf, c] = doubt
            if found and not doubt:
                seen_it[leaf, c] = True
                votes[leaf, :3] += rgba[leaf, :3].astype(np.int64)
                votes[leaf, 3] += 1
    return dict(votes=votes, candidate=candidate, visible=seen_it, undecided=unsure,
                pairs=count * cameras)


def colors(votes, before):
    """(L,3) f32: ``sum / (float)(255 count)``, one f32 division of two exact integers, where
    ``count > 0``; ``before`` elsewhere."""
    votes = np.asarray(votes, np.int64)
    out = np.array(before, F, copy=True)
    some = votes[:, 3] > 0
    assert (255 * votes[:, 3]).max(initial=0) <= 2 ** 24
    denominator = (255 * votes[some, 3]).astype(F)
    for ch in range(3):
        out[some, ch] = (votes[some, ch].astype(F) / denominator).astype(F)
    return out
