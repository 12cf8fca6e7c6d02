"""Octree fixtures FROM THE REFERENCE ITSELF -> octree.npz, and the reference voxelize_model.py
parser -> cli_defaults_voxelize.json.  Build container only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_octree.py

The reference's octree runs as plain Python under the inert stand-ins of
make_goldens._install_stubs() (numba.njit is the identity).  Recorded per cloud (data, not
source): the inputs, and the reference's node_index, leaf_index, scale, leaf_data, leaf_centers,
leaf_depths, its answers to a set of query points, and the pruned tree.  Only cases the
reference completes are taken: the root-only cloud records the tree arrays alone (the reference
reports a stand-in leaf for it and its query fails), and no cloud has depth 1 with fewer than
min_leaf_size points."""

import contextlib
import importlib.util
import io
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CLI_ARGV = ["model.pt", "data.npz", "out.npz"]


def clouds():
    """name -> (positions f32 (N,3), depth, min_leaf_size, data f32 (N,C) or None)."""
    rng = np.random.default_rng(20080524)
    out = {}
    n = 20000
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    shell = (d * (0.6 + 0.02 * rng.normal(size=(n, 1))) + [0.1, -0.05, 0.2]).astype(np.float32)
    out["shell"] = (shell, 6, 4, rng.random((n, 3)).astype(np.float32))
    # every coordinate a dyadic multiple of the extent: points on splitting planes and cube faces
    grid = rng.integers(0, 33, size=(6000, 3)).astype(np.float32) / 32 * 2 - 1
    grid = np.concatenate([grid, [[-1, -1, -1], [1, 1, 1], [0, 0, 0], [1, -1, 0]]]).astype(np.float32)
    out["planes"] = (grid, 5, 3, rng.random((len(grid), 3)).astype(np.float32))
    out["tiny"] = (rng.normal(size=(3, 3)).astype(np.float32), 4, 4,
                   rng.random((3, 2)).astype(np.float32))
    out["depth1"] = (rng.normal(size=(500, 3)).astype(np.float32), 1, 4,
                     rng.random((500, 3)).astype(np.float32))
    blob = (rng.normal(size=(4000, 3)) * [0.5, 0.2, 0.1]).astype(np.float32)
    out["nodata"] = (blob, 5, 2, None)
    return out


def queries(rng, scale, positions, center):
    q = (rng.random((3000, 3)) * 2.6 - 1.3) * scale
    on_planes = rng.integers(-8, 9, size=(600, 3)) / 8 * scale
    own = positions[:400] - center
    return np.concatenate([q, on_planes, own]).astype(np.float32)


def main():
    sys.path.insert(0, HERE)
    from make_goldens import REFERENCE, _install_stubs
    _install_stubs()
    sys.path.insert(0, REFERENCE)
    sys.dont_write_bytecode = True
    import fourier_feature_nets as ffn

    spec = importlib.util.spec_from_file_location("ref_voxelize_model",
                                                  os.path.join(REFERENCE, "voxelize_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    old = sys.argv
    sys.argv = ["voxelize_model.py"] + CLI_ARGV
    try:
        cli = {"voxelize_model": vars(mod._parse_args())}
    finally:
        sys.argv = old
    with open(os.path.join(HERE, "cli_defaults_voxelize.json"), "w") as f:
        json.dump(cli, f, indent=1, sort_keys=True)

    rng = np.random.default_rng(7)
    out = {"names": np.array(sorted(clouds()))}
    for name, (positions, depth, min_leaf, data) in clouds().items():
        center = 0.5 * (positions.min(0) + positions.max(0))
        with contextlib.redirect_stdout(io.StringIO()):
            tree = ffn.OcTree.build_from_samples(positions.copy(), depth, min_leaf,
                                                 None if data is None else data.copy())
        out[name + "/positions"] = positions
        out[name + "/depth"] = np.int64(depth)
        out[name + "/min_leaf_size"] = np.int64(min_leaf)
        if data is not None:
            out[name + "/data"] = data
            out[name + "/leaf_data"] = tree.leaf_data()
        state = tree.state_dict
        out[name + "/node_index"] = np.asarray(state["node_index"], np.int64)
        out[name + "/leaf_index"] = np.asarray(state["leaf_index"], np.int64)
        out[name + "/scale"] = np.float32(state["scale"])
        assert np.float32(state["scale"]) == state["scale"]
        if len(state["node_index"]) == 0:
            continue                    # root only: a stand-in leaf, and query fails there
        out[name + "/leaf_centers"] = tree.leaf_centers()
        out[name + "/leaf_depths"] = tree.leaf_depths()
        q = queries(rng, np.float32(state["scale"]), positions, center)
        try:
            out[name + "/query_result"] = tree.query(q)
            out[name + "/query"] = q
        except (IndexError, TypeError):
            # the reference runs off the end of leaf_index for some positions: keep the ones it
            # answers
            keep, answers = [], []
            for p in q:
                try:
                    answers.append(int(tree.query(p)[0]))
                    keep.append(p)
                except (IndexError, TypeError):
                    pass
            out[name + "/query"] = np.array(keep, np.float32)
            out[name + "/query_result"] = np.array(answers, np.int64)
        with contextlib.redirect_stdout(io.StringIO()):
            pruned = tree.prune()
        ps = pruned.state_dict
        out[name + "/pruned_node_index"] = np.asarray(ps["node_index"], np.int64)
        out[name + "/pruned_leaf_index"] = np.asarray(ps["leaf_index"], np.int64)
        if data is not None:
            out[name + "/pruned_leaf_data"] = pruned.leaf_data()
    np.savez_compressed(os.path.join(HERE, "octree.npz"), **out)
    for key in sorted(out):
        print(key, getattr(out[key], "shape", None), getattr(out[key], "dtype", None))


if __name__ == "__main__":
    main()
