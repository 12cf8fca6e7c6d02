"""Ray paths FROM THE REFERENCE ITSELF -> octree_walk.npz.  Build container only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_octree_walk.py

The reference's ``OcTree.intersect`` (octree.py:418-501, 707-731) runs as plain Python under the
inert stand-ins of make_goldens._install_stubs() (numba.njit is the identity, so its arithmetic
is numpy f32 scalars), on the ``shell``, ``planes`` and ``nodata`` trees that it builds from the
clouds of octree.npz.  Recorded per tree (data, not source): the rays and, at ``max_length`` 64
and at a ``max_length`` that truncates, the ``t_stops`` and ``leaves`` it returns.

Rays: camera-like ones from outside the cube, rays that start inside it, rays that point away
from it (the cube behind them, or missed altogether); unit and non-unit directions, every component nonzero (the reference replaces zeros, octree.py:728).

One stand-in beyond the stubs: the reference reads ``leaf_index[searchsorted(...)]`` without a
bound (octree.py:451), which is an IndexError in plain Python for an empty cell whose id is above
every leaf id.  For the ``intersect`` calls its ``_leaf_index`` gets one sentinel id (2^62)
appended; no real id equals it and the recorded indices are unchanged.

The reference advances by 1e-5 nudges, so it has no answer that a walk defined by plane crossings
could reproduce on a ray that cuts a region in a chord of a few nudges.  Such GRAZING rays (margin
of tests/octree_walk_reference.py below 4e-5) are left out by the test; this generator asserts
that they are at most 10 % of each fixture's rays, that the reference's leaf sequence equals the
restatement's on all the others, and records, per fixture, the largest ``reference t - crossing
t`` it saw (``max_excess``): the test allows the reference twice that."""

import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TREES = ["shell", "planes", "nodata"]
LENGTHS = [64, 6]
GRAZING = 4e-5
CAP = 0.10


def rays(rng, scale):
    """starts, directions f32 (N,3) in the tree's frame."""
    def unit(v):
        return v / np.linalg.norm(v, axis=1, keepdims=True)

    n_out, n_in, n_miss = 700, 300, 200
    eye = unit(rng.normal(size=(n_out, 3))) * scale * rng.uniform(2.0, 4.0, size=(n_out, 1))
    target = (rng.random((n_out, 3)) * 2 - 1) * scale * 0.95
    out_d = unit(target - eye)
    inside = (rng.random((n_in, 3)) * 2 - 1) * scale * 0.9
    in_d = unit(rng.normal(size=(n_in, 3)))
    away = unit(rng.normal(size=(n_miss, 3)))
    miss_o = away * scale * rng.uniform(2.0, 4.0, size=(n_miss, 1))
    # pointing away from the cube: some of these lines miss it altogether, the others cross it
    # at negative t only (the reference does not return on some rays whose line passes the cube
    # sideways at a distance; those cannot be recorded)
    miss_d = unit(away + 0.3 * rng.normal(size=(n_miss, 3)))
    starts = np.concatenate([eye, inside, miss_o])
    directions = np.concatenate([out_d, in_d, miss_d])
    # every other ray: a direction that is not of unit length
    directions[1::2] *= rng.uniform(0.25, 2.0, size=(len(directions[1::2]), 1))
    starts, directions = starts.astype(np.float32), directions.astype(np.float32)
    assert (directions != 0).all()
    return starts, directions


def main():
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from make_goldens import REFERENCE, _install_stubs
    _install_stubs()
    sys.path.insert(0, REFERENCE)
    sys.dont_write_bytecode = True
    import fourier_feature_nets as ffn
    from tests import octree_walk_reference as wref

    with np.load(os.path.join(HERE, "octree.npz")) as g:
        clouds = {k: g[k] for k in g.files}
    rng = np.random.default_rng(418501)
    out = {"names": np.array(TREES), "lengths": np.array(LENGTHS, np.int64),
           "grazing": np.float64(GRAZING)}
    for name in TREES:
        data = clouds.get(name + "/data")
        with contextlib.redirect_stdout(io.StringIO()):
            tree = ffn.OcTree.build_from_samples(clouds[name + "/positions"].copy(),
                                                 int(clouds[name + "/depth"]),
                                                 int(clouds[name + "/min_leaf_size"]),
                                                 None if data is None else data.copy())
        state = tree.state_dict
        node_index = np.asarray(state["node_index"], np.int64)
        leaf_index = np.asarray(state["leaf_index"], np.int64)
        assert np.array_equal(leaf_index, clouds[name + "/leaf_index"])
        assert np.array_equal(node_index, clouds[name + "/node_index"])
        scale = np.float32(state["scale"])
        tree._leaf_index = np.append(leaf_index, np.int64(2 ** 62))
        starts, directions = rays(rng, scale)
        out[name + "/starts"], out[name + "/directions"] = starts, directions
        exact = wref.walk(scale, node_index, leaf_index, starts, directions)
        grazing = exact["margin"] < GRAZING
        assert grazing.mean() <= CAP, (name, grazing.mean())
        excess = 0.0
        for length in LENGTHS:
            got = tree.intersect(starts.copy(), directions.copy(), length)
            t_stops = np.asarray(got.t_stops, np.float32)
            leaves = np.asarray(got.leaves, np.int64)
            assert t_stops.shape == (len(starts), length) and leaves.max() < len(leaf_index)
            out["%s/t_stops_%d" % (name, length)] = t_stops
            out["%s/leaves_%d" % (name, length)] = leaves
            want_t, want_leaves, written = wref.path(exact, length)
            ok = ~grazing
            assert np.array_equal(leaves[ok], want_leaves[ok]), name
            live = ok[:, None] & (np.arange(length)[None, :] < written[:, None])
            excess = max(excess, float((t_stops.astype(np.float64) - want_t)[live].max()))
        out[name + "/max_excess"] = np.float64(excess)
        print(name, "rays", len(starts), "grazing %.4f" % grazing.mean(), "hit %.3f" %
              exact["hit"].mean(), "max excess %.3g" % excess)
    np.savez_compressed(os.path.join(HERE, "octree_walk.npz"), **out)
    print(os.path.getsize(os.path.join(HERE, "octree_walk.npz")), "bytes")


if __name__ == "__main__":
    main()
