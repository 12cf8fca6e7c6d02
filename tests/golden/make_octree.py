"""Octree fixtures FROM THE REFERENCE ITSELF -> octree.npz and octree_edges.npz, and the reference
voxelize_model.py parser -> cli_defaults_voxelize.json.  Build container only:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_octree.py            # everything
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_octree.py edges      # octree_edges.npz alone

octree_edges.npz (``edge_clouds`` and ``chain_tree``) holds the degenerate clouds and the deepest
tree an int64 id allows; it was added after octree.npz, which is left as it was recorded.

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


def edge_clouds():
    """The clouds of octree_edges.npz: name -> (positions, depth, min_leaf_size, data or None)."""
    rng = np.random.default_rng(20240611)
    f32 = np.float32
    out = {}
    out["identical"] = (np.tile(f32([[0.3, -1.7, 2.5]]), (40, 1)), 6, 4,
                        rng.random((40, 3)).astype(f32))
    out["single_point"] = (f32([[0.5, 0.25, -3.0]]), 4, 1, None)
    out["two_points"] = (f32([[0, 0, 0], [1, 1, 1]]), 11, 1, rng.random((2, 2)).astype(f32))
    segment = np.zeros((257, 3), f32)
    segment[:, 0] = np.linspace(-1, 1, 257)
    out["segment"] = (segment, 9, 2, None)
    plane = (rng.random((3000, 3)) * 2 - 1).astype(f32)
    plane[:, 2] = 0.25
    out["plane"] = (plane, 7, 3, rng.random((3000, 4)).astype(f32))
    uniform = (rng.random((2000, 3)) * 2 - 1).astype(f32)
    out["depth11_dupes"] = (np.concatenate([np.tile(uniform[:1], (50, 1)), uniform]), 11, 3,
                            rng.random((2050, 3)).astype(f32))
    out["depth11_min1"] = ((rng.random((3000, 3)) * 2 - 1).astype(f32), 11, 1, None)
    out["min_equals_n"] = ((rng.random((64, 3)) * 2 - 1).astype(f32), 5, 64, None)
    k = np.arange(17, dtype=f32) / f32(8) - f32(1)
    out["lattice17"] = (np.stack(np.meshgrid(k, k, k, indexing="ij"), -1).reshape(-1, 3), 6, 1,
                        rng.random((17 ** 3, 2)).astype(f32))
    k = f32(0.3) * np.arange(9, dtype=f32) / f32(8)
    lattice = np.stack(np.meshgrid(k, k, k, indexing="ij"), -1).reshape(-1, 3)
    out["offcentre_lattice"] = ((lattice + f32([0.1, 0.7, -0.3])).astype(f32), 5, 2, None)
    return out


CHAIN_LEVELS = 20
CHAIN_SCALE = np.float32(0.7)


def chain_tree():
    """-> node ids, leaf ids (sorted int64).  At every level 0 .. 19 one node is interior; its child
    ``(3 level) % 8`` is the interior node of the next level and the other seven are leaves; all
    eight children of the level-19 node are leaves, at level 20: the deepest id an int64 holds."""
    nodes, leaves, node = [], [], 0
    for level in range(CHAIN_LEVELS):
        nodes.append(node)
        for child in range(8):
            if child != (3 * level) % 8 or level == CHAIN_LEVELS - 1:
                leaves.append(8 * node + 1 + child)
        node = 8 * node + 1 + (3 * level) % 8
    return np.array(sorted(nodes), np.int64), np.array(sorted(leaves), np.int64)


def chain_queries(rng, scale, centers):
    """Every leaf centre, each centre one f32 step up and down per axis, 500 dyadic multiples of
    the scale, 500 random positions a little beyond the cube."""
    steps = []
    for axis in range(3):
        for toward in (-np.inf, np.inf):
            moved = centers.copy()
            moved[:, axis] = np.nextafter(centers[:, axis], np.float32(toward))
            steps.append(moved)
    dyadic = (rng.integers(-64, 65, size=(500, 3)) / 64).astype(np.float32) * scale
    q = ((rng.random((500, 3)) * 2.2 - 1.1) * scale)
    return np.concatenate([centers] + steps + [dyadic, q]).astype(np.float32)


def answered(tree, q):
    """The positions of q the reference answers (it runs off the end of leaf_index for some), and
    its answers."""
    try:
        return q, tree.query(q)
    except (IndexError, TypeError):
        keep, answers = [], []
        for p in q:
            try:
                answers.append(int(tree.query(p)[0]))
                keep.append(p)
            except (IndexError, TypeError):
                pass
        return np.array(keep, np.float32), np.array(answers, np.int64)


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

    if "edges" not in sys.argv[1:]:
        out = record_clouds(ffn, clouds(), np.random.default_rng(7))
        np.savez_compressed(os.path.join(HERE, "octree.npz"), **out)
        show(out)
    out = record_clouds(ffn, edge_clouds(), np.random.default_rng(8))
    # The deep chain is a hand-written state dict.  It is handed to the reference's constructor
    # with the np.float32 scale a tree built by build_from_samples carries, so that the node
    # centres are the f32 chain (OcTree.load would turn the scale into a Python float, and the
    # reference would then descend in f64: see the notes of fourier_feature_nets_amd/octree.py).
    node_index, leaf_index = chain_tree()
    with contextlib.redirect_stdout(io.StringIO()):
        tree = ffn.OcTree(CHAIN_SCALE, set(node_index.tolist()), set(leaf_index.tolist()))
    assert type(tree.leaves[-1].x) is np.float32
    out["chain/node_index"], out["chain/leaf_index"] = node_index, leaf_index
    assert np.array_equal(tree.state_dict["leaf_index"], leaf_index)
    out["chain/scale"] = CHAIN_SCALE
    out["chain/leaf_centers"] = tree.leaf_centers()
    out["chain/leaf_depths"] = tree.leaf_depths()
    out["chain/query"], out["chain/query_result"] = answered(
        tree, chain_queries(np.random.default_rng(9), CHAIN_SCALE, tree.leaf_centers()))
    np.savez_compressed(os.path.join(HERE, "octree_edges.npz"), **out)
    show(out)


def show(out):
    for key in sorted(out):
        print(key, getattr(out[key], "shape", None), getattr(out[key], "dtype", None))


def record_clouds(ffn, cloud_set, rng):
    out = {"names": np.array(sorted(cloud_set))}
    for name, (positions, depth, min_leaf, data) in cloud_set.items():
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
        out[name + "/query"], out[name + "/query_result"] = answered(tree, q)
        with contextlib.redirect_stdout(io.StringIO()):
            pruned = tree.prune()
        ps = pruned.state_dict
        out[name + "/pruned_node_index"] = np.asarray(ps["node_index"], np.int64)
        out[name + "/pruned_leaf_index"] = np.asarray(ps["leaf_index"], np.int64)
        if data is not None:
            out[name + "/pruned_leaf_data"] = pruned.leaf_data()
    return out

if __name__ == "__main__":
    main()
