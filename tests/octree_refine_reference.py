"""Restatements for the K21 tests (CPU and GPU), written from the contract in include/ffn_hip.h.

``leaf_max_weights``: the float64 per-leaf maximum of the compositing weights that
``tests/octree_volume_reference.composite`` gives the taken crossings, and per leaf the tolerance
of the comparison: the largest ``budget_a`` of the rays that take the leaf.  That tolerance is
derived, not tuned: a weight ``T_k a_k`` of a ray moves by no more than the ray's alpha budget
under the perturbations the budget covers, and ``|max x - max y| <= max |x - y|``.

``refine``: drop / keep / split on sorted ids in plain numpy.  The result is sorted by id, so the
order in which the leaves are visited does not matter here (the kernel works in path-code order
because K12h wants it)."""

import numpy as np

from tests import octree_volume_reference as vref

DROP, KEEP, SPLIT = 0, 1, 2


def leaf_max_weights(w, scale, starts, directions, leaf_data, num_leaves, t_min=0.0,
                     min_transmittance=0.0):
    """``w``: a ``octree_walk_reference.walk`` result; ``leaf_data`` (L, C >= 4) with the density in
    column 3.  -> weights (L,) float64, budget (L,) float64, taken (L,) bool (some ray takes the
    leaf), and the ``composite`` dict."""
    v = vref.composite(w, scale, starts, directions, leaf_data, t_min, (0.0, 0.0, 0.0),
                       min_transmittance)
    leaf = w["leaf"][v["taken"]]
    ray = w["ray"][v["taken"]]
    weights = np.zeros(num_leaves)
    budget = np.zeros(num_leaves)
    taken = np.zeros(num_leaves, bool)
    np.maximum.at(weights, leaf, v["weights"])
    np.maximum.at(budget, leaf, v["budget_a"][ray])
    taken[leaf] = True
    return weights, budget, taken, v


def id_levels(ids):
    ids = np.asarray(ids, np.int64).copy()
    level = np.zeros(ids.shape, np.int64)
    while (ids > 0).any():
        live = ids > 0
        level[live] += 1
        ids[live] = (ids[live] - 1) >> 3
    return level


def ancestors(leaf_ids):
    """The sorted ids of every proper ancestor of the given nodes."""
    nodes = set()
    for node in np.asarray(leaf_ids, np.int64).tolist():
        while node > 0:
            node = (node - 1) >> 3
            if node in nodes:
                break
            nodes.add(node)
    return np.array(sorted(nodes), np.int64)


def refine(leaf_index, rows, action):
    """``leaf_index`` (L,) sorted ids, ``rows`` (L,C) or None, ``action`` (L,) of 0 / 1 / 2.
    -> leaf_index, node_index, rows, parent of the new tree, sorted by id."""
    leaf_index = np.asarray(leaf_index, np.int64)
    action = np.asarray(action)
    assert action.shape == leaf_index.shape and (action <= SPLIT).all()
    ids, parent = [], []
    for number, (node, act) in enumerate(zip(leaf_index.tolist(), action.tolist())):
        if act == KEEP:
            ids.append(node)
            parent.append(number)
        elif act == SPLIT:
            ids.extend(8 * node + 1 + child for child in range(8))
            parent.extend([number] * 8)
    ids, parent = np.array(ids, np.int64), np.array(parent, np.int64)
    order = np.argsort(ids, kind="stable")
    ids, parent = ids[order], parent[order]
    assert len(np.unique(ids)) == len(ids)
    return ids, ancestors(ids), None if rows is None else np.asarray(rows)[parent], parent
