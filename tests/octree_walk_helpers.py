"""Small fixtures shared by the K13 ray-walk tests (CPU and GPU)."""

import numpy as np

from tests import octree_walk_reference as wref

LEFT_OUT_CAP = 0.02


def two_level_tree():
    """Root (interior) with children 1 (leaf), 8 (interior; its children 65 and 72 leaves);
    scale 1.  Child index 4 [x >= 0] + 2 [y >= 0] + [z >= 0]: node 1 is the (-,-,-) octant,
    node 8 the (+,+,+) octant, 65 / 72 its (-,-,-) / (+,+,+) corners.
    -> scale, node_index, leaf_index."""
    return np.float32(1.0), np.array([0, 8], np.int64), np.array([1, 65, 72], np.int64)


def opaque_ball(side=16):
    """A Voxels model with an opaque ball of radius 0.45 in empty space (the model that
    tests/test_octree_gpu.py voxelizes): rays through it end with alpha ~ 1, the others ~ 0."""
    import torch
    import fourier_feature_nets as ffn
    model = ffn.Voxels(side, 1.0)
    axis = (np.arange(side) + 0.5) / side * 2 - 1
    x, y, z = np.meshgrid(axis, axis, axis, indexing="ij")
    inside = x * x + y * y + z * z < 0.45 ** 2
    volume = np.random.default_rng(3).normal(size=(1, 4, side, side, side)).astype(np.float32)
    volume[0, 3] = np.where(inside, 12.0, -12.0)
    with torch.no_grad():
        model.voxels.copy_(torch.from_numpy(volume))
        model.bias.zero_()
    return model


def ray_budget(w, scale, starts, directions):
    """Per ray: the largest crossing budget, and the same expression for the planes that do not
    show up as a crossing (a near miss is decided on them too): the cube's extent, the ray's
    smallest nonzero direction component."""
    _, _, per_ray = wref.budgets(w, scale, starts, directions)
    o = np.abs(np.asarray(starts, np.float64)).max(1)
    d = np.abs(np.asarray(directions, np.float64))
    d_min = np.where(d > 0, d, np.inf).min(1)
    t_max = np.maximum(np.abs(w["root_in"]), np.abs(w["root_out"]))
    t_max = np.where(np.isfinite(t_max), t_max, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        wide = 4 * (np.spacing(np.float32(np.float64(scale) + o)).astype(np.float64) / d_min
                    + np.spacing(t_max.astype(np.float32)).astype(np.float64))
    return np.maximum(per_ray, np.where(np.isfinite(wide), wide, np.inf))


def check_walk(what, state, starts, directions, length, got_t, got_leaves):
    scale, nodes, leaves = state["scale"], state["node_index"], state["leaf_index"]
    w = wref.walk(scale, nodes, leaves, starts, directions)
    want_t, want_leaves, written = wref.path(w, length)
    entry, _, _ = wref.budgets(w, scale, starts, directions)
    budget = ray_budget(w, scale, starts, directions)
    ok = ~w["hit"] | (w["margin"] > budget)
    left_out = 1.0 - ok.mean()
    same = (got_leaves == want_leaves).all(1)
    print("%s L=%d: %d rays, %.4f left out, %d of them differ, longest path %d" %
          (what, length, len(ok), left_out, (~same & ~ok).sum(), np.diff(w["offsets"]).max()))
    assert got_t.dtype == np.float32 and got_leaves.dtype == np.int64
    assert got_t.shape == (len(ok), length) and got_leaves.shape == (len(ok), length)
    assert left_out <= LEFT_OUT_CAP
    assert same[ok].all()
    assert (got_leaves[~w["hit"]] == -1).all()
    # entry t, stop by stop, and the fill
    stop_budget = np.zeros((len(ok), length))
    k = np.arange(len(w["ray"])) - w["offsets"][w["ray"]]
    keep = k < length - 1
    stop_budget[w["ray"][keep], k[keep]] = entry[keep]
    column = np.arange(length)[None, :]
    rows = (ok & w["hit"])[:, None]
    live = rows & (column < written[:, None])
    fill = rows & (column >= written[:, None])
    err = np.abs(got_t.astype(np.float64) - want_t)
    with np.errstate(invalid="ignore"):
        print("   worst entry error / budget %.3f" % (err[live] / stop_budget[live]).max())
    assert (err <= stop_budget)[live].all()
    assert (err <= budget[:, None])[fill].all()
    return w, ok
