"""The op-by-op restatement of the K12 build (tests/octree_reference.py) against the trees the
reference built (tests/golden/octree.npz, octree_edges.npz), the hand cases of
tests/octree_build_helpers.py against the restatement, and the TEETH of the helper inputs: each
way a kernel could be subtly wrong is applied to a copy of the restatement here, on the CPU, and
must change the answer on the inputs tests/test_octree_build_ops_gpu.py feeds the kernels."""

import os

import numpy as np
import pytest

from tests import octree_build_helpers as hp
from tests import octree_reference as oref

HERE = os.path.dirname(os.path.abspath(__file__))
EDGE_CLOUDS = ["identical", "single_point", "two_points", "segment", "plane", "depth11_dupes",
               "depth11_min1", "min_equals_n", "lattice17", "offcentre_lattice"]
OLD_CLOUDS = ["shell", "planes", "tiny", "depth1", "nodata"]


def load(name):
    with np.load(os.path.join(HERE, "golden", name)) as g:
        return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def golden():
    return {"octree.npz": load("octree.npz"), "octree_edges.npz": load("octree_edges.npz")}


def cloud(g, name):
    return {k.split("/", 1)[1]: v for k, v in g.items() if k.startswith(name + "/")}


ALL_CLOUDS = [("octree.npz", n) for n in OLD_CLOUDS] + [("octree_edges.npz", n) for n in EDGE_CLOUDS]


def id_depth(ids):
    return oref.leaf_geometry(1.0, np.asarray(ids, np.int64))[1]


def test_fixture_covers_the_cases(golden):
    g = golden["octree_edges.npz"]
    assert set(str(n) for n in g["names"]) == set(EDGE_CLOUDS)
    assert os.path.getsize(os.path.join(HERE, "golden", "octree_edges.npz")) < \
        os.path.getsize(os.path.join(HERE, "golden", "octree.npz"))
    assert g["identical/scale"] == 0 and g["identical/scale"].dtype == np.float32
    assert len(g["identical/leaf_index"]) == 1 and id_depth(g["identical/leaf_index"])[0] == 5
    assert g["single_point/scale"] == 0 and id_depth(g["single_point/leaf_index"])[0] == 3
    for name in ("two_points", "depth11_dupes", "depth11_min1"):
        assert int(g[name + "/depth"]) == 11 and id_depth(g[name + "/leaf_index"]).max() == 10
    assert len(g["min_equals_n/node_index"]) == 0 and list(g["min_equals_n/leaf_index"]) == [0]
    for name in ("segment", "plane", "depth11_dupes", "offcentre_lattice"):
        c = cloud(g, name)
        mine = oref.build(c["positions"], int(c["depth"]), int(c["min_leaf_size"]))
        assert (mine["point_leaf"] < 0).any(), name
    assert sum(name + "/data" in g for name in EDGE_CLOUDS) == 5
    for name in EDGE_CLOUDS:
        if name + "/data" in g:
            assert 2 <= g[name + "/data"].shape[1] <= 4
    # the chain: one interior node per level 0 .. 19, eight leaves at level 20
    depths = id_depth(g["chain/leaf_index"])
    assert depths.max() == 20 and (depths == 20).sum() == 8 and len(depths) == 19 * 7 + 8
    assert np.array_equal(depths, g["chain/leaf_depths"])
    assert len(g["chain/node_index"]) == 20 and g["chain/scale"] == np.float32(0.7)
    assert len(g["chain/query"]) >= 141 * 7 + 900
    assert (g["chain/query_result"] >= 0).sum() > 141 * 4 and (g["chain/query_result"] < 0).any()
    # the additions of scale / 2^k round: the f32 chain is not the exact sum
    exact, half = np.zeros(3), float(g["chain/scale"])
    leaf = int(g["chain/leaf_index"][-1])
    digits = []
    while leaf > 0:
        digits.append((leaf - 1) & 7)
        leaf = (leaf - 1) >> 3
    for d in digits[::-1]:
        half /= 2
        exact += np.where([d & 4, d & 2, d & 1], half, -half)
    assert (exact.astype(np.float32) != g["chain/leaf_centers"][-1]).any()


def rebuilt(c):
    """path_codes -> stable sort -> structure_from_codes -> interior_nodes on a cloud."""
    center, scale = oref.root_cube(c["positions"])
    depth = int(c["depth"])
    codes = oref.path_codes(c["positions"], center, scale, depth)
    perm = np.argsort(codes, kind="stable")
    leaf, leaves = oref.structure_from_codes(codes[perm], depth, int(c["min_leaf_size"]))
    point_leaf = np.empty(len(codes), np.int64)
    point_leaf[perm] = leaf
    return dict(scale=scale, codes=codes, perm=perm, leaves=leaves, point_leaf=point_leaf,
                leaf_index=np.sort(leaves[:, 0]), node_index=oref.interior_nodes(leaves[:, 0]))


@pytest.mark.parametrize("file,name", ALL_CLOUDS)
def test_the_ops_chained_reproduce_the_reference_trees(golden, file, name):
    c = cloud(golden[file], name)
    mine = rebuilt(c)
    assert np.array_equal(mine["leaf_index"], c["leaf_index"])
    assert np.array_equal(mine["node_index"], c["node_index"])
    assert np.float32(mine["scale"]).tobytes() == c["scale"].tobytes()
    whole = oref.build(c["positions"], int(c["depth"]), int(c["min_leaf_size"]), c.get("data"))
    assert np.array_equal(mine["point_leaf"], whole["point_leaf"])
    assert np.array_equal(whole["leaf_index"], c["leaf_index"])
    assert np.array_equal(whole["node_index"], c["node_index"])
    # (id, start, count): the counts are the leaves' point counts, the runs tile the kept points
    order = np.argsort(mine["leaves"][:, 0])
    assert np.array_equal(mine["leaves"][order, 2], whole["leaf_count"])
    assert mine["leaves"][:, 2].sum() == (mine["point_leaf"] >= 0).sum()
    if "leaf_centers" in c:
        centers, depths = oref.leaf_geometry(c["scale"], c["leaf_index"])
        assert centers.tobytes() == c["leaf_centers"].tobytes()
        assert np.array_equal(depths, c["leaf_depths"])
    if "query" in c:
        assert np.array_equal(oref.query(c["scale"], c["node_index"], c["leaf_index"], c["query"]),
                              c["query_result"])


def test_restatement_answers_the_deep_chain_as_the_reference_does(golden):
    g = cloud(golden["octree_edges.npz"], "chain")
    centers, depths = oref.leaf_geometry(g["scale"], g["leaf_index"])
    assert centers.tobytes() == g["leaf_centers"].tobytes()
    assert np.array_equal(depths, g["leaf_depths"])
    answers = oref.query(g["scale"], g["node_index"], g["leaf_index"], g["query"])
    assert np.array_equal(answers, g["query_result"])
    assert np.array_equal(oref.interior_nodes(g["leaf_index"]), g["node_index"])
    # every leaf centre answers its own leaf
    assert np.array_equal(answers[:len(centers)], np.arange(len(centers)))


@pytest.mark.parametrize("name", sorted(hp.structure_cases()))
def test_hand_cases_equal_the_restatement(name):
    case = hp.structure_cases()[name]
    leaf, leaves = oref.structure_from_codes(case["codes"], case["depth"], case["min_leaf_size"])
    assert np.array_equal(leaf, case["leaf"])
    assert np.array_equal(leaves, case["leaves"])


def test_surface_points_keep_ray_order_and_a_strict_threshold():
    inp = hp.surface_inputs(300)
    flags = hp.flag_pattern("half", 300)
    alpha = hp.alpha_from_flags(flags)
    assert (alpha == np.float32(hp.THRESHOLD)).sum() > 10
    pos, col = oref.surface_points(alpha, inp["depth"], inp["starts"], inp["directions"],
                                   inp["color"], hp.THRESHOLD)
    assert len(pos) == flags.sum() and pos.dtype == np.float32
    assert np.array_equal(col[:, 0], np.flatnonzero(flags))          # the rows name their rays


# ------------------------------------------------------------------------------------ teeth
def codes_with(positions, center, scale, depth, strict=False, shift_centre=False):
    """oref.path_codes with one thing wrong."""
    positions = np.asarray(positions, np.float32)
    center = np.asarray(center, np.float32)
    points = positions if shift_centre else (positions - center).astype(np.float32)
    centers = np.tile(center, (len(points), 1)) if shift_centre else np.zeros_like(points)
    half, codes = np.float32(scale), np.zeros(len(points), np.int64)
    for _ in range(1, depth):
        half = np.float32(half / np.float32(2))
        side = points > centers if strict else points >= centers
        codes = codes * 8 + side[:, 0] * 4 + side[:, 1] * 2 + side[:, 2]
        centers = np.where(side, centers + half, centers - half).astype(np.float32)
    return codes


def test_teeth_path_codes():
    for center, scale in hp.CUBES:
        positions = hp.path_code_positions(center, scale)
        for depth in range(1, hp.MAX_DEPTH + 1):
            right = oref.path_codes(positions, center, scale, depth)
            assert np.array_equal(codes_with(positions, center, scale, depth), right)
            if depth > 1:
                assert (codes_with(positions, center, scale, depth, strict=True) != right).any()
    center, scale = hp.CUBES[0]
    positions = hp.path_code_positions(center, scale)
    # (at depth 2 the two are the same: x - c >= 0 iff x >= c in IEEE arithmetic)
    for depth in range(3, hp.MAX_DEPTH + 1):
        wrong = codes_with(positions, center, scale, depth, shift_centre=True)
        assert (wrong != oref.path_codes(positions, center, scale, depth)).any(), depth
    # the specials are there: NaN, both infinities, a negative zero, points outside
    p = hp.path_code_positions(*hp.CUBES[1])
    assert np.isnan(p).any() and np.isposinf(p).any() and np.isneginf(p).any()
    assert (np.signbit(p) & (p == 0)).any() and (np.abs(p) > 1).any() and (np.abs(p) == 1).any()
    # all 30 bits of a depth-11 code are used
    assert oref.path_codes(p, (0, 0, 0), 1.0, 11).max() == 8 ** 10 - 1


def structure_with(codes, depth, min_leaf, inclusive=False, always_leaf=False):
    """oref.structure_from_codes's leaf per point with one thing wrong."""
    codes = np.asarray(codes, np.int64)
    n = len(codes)
    leaf, ids = np.full(n, -1, np.int64), np.zeros(n, np.int64)
    alive = np.full(n, depth > 1 or (n > min_leaf if inclusive else n >= min_leaf))
    for level in range(1, depth):
        child = codes >> (3 * (depth - 1 - level))
        _, inverse, counts = np.unique(child[alive], return_inverse=True, return_counts=True)
        followed = np.zeros(n, bool)
        followed[alive] = counts[inverse] > min_leaf if inclusive else counts[inverse] >= min_leaf
        interior = alive & np.isin(child >> 3, np.unique(child[followed] >> 3))
        leaf_here = alive & ~followed if always_leaf else alive & ~interior
        leaf[leaf_here] = ids[leaf_here]
        alive = followed
        ids = np.where(alive, 8 * ids + 1 + (child & 7), ids)
    leaf[alive] = ids[alive]
    return leaf


def test_teeth_structure():
    cases = hp.structure_cases()
    caught = {"inclusive": [], "always_leaf": []}
    for name, case in cases.items():
        args = (case["codes"], case["depth"], case["min_leaf_size"])
        assert np.array_equal(structure_with(*args), case["leaf"]), name
        for kind in caught:
            if not np.array_equal(structure_with(*args, **{kind: True}), case["leaf"]):
                caught[kind].append(name)
    assert {"starved_siblings_depth2", "starved_siblings_depth3", "no_followed_child",
            "chain_to_the_last_level", "min_leaf_is_n", "min_leaf_is_n_at_depth_1"} \
        <= set(caught["inclusive"])
    assert {"starved_siblings_depth2", "starved_siblings_depth3", "no_followed_child",
            "chain_to_the_last_level"} <= set(caught["always_leaf"])


def scan_without_carry(flags):
    """The three-kernel scan with the carry between groups of 256 tile sums forgotten."""
    n = len(flags)
    tiles = -(-n // hp.SCAN_TILE)
    padded = np.zeros(tiles * hp.SCAN_TILE, np.int64)
    padded[:n] = flags
    per_tile = padded.reshape(tiles, hp.SCAN_TILE)
    sums = per_tile.sum(1)
    prefix = np.zeros(tiles, np.int64)
    for first in range(0, tiles, 256):                       # each group starts again from zero
        group = sums[first:first + 256]
        prefix[first:first + 256] = np.cumsum(group) - group
    within = np.cumsum(per_tile, 1) - per_tile
    return (within + prefix[:, None]).reshape(-1)[:n]


def test_teeth_scan():
    for n in hp.SCAN_SIZES:
        for name in hp.FLAG_PATTERNS:
            flags = hp.flag_pattern(name, n)
            assert flags.shape == (n,) and flags.dtype == bool
            right, total = hp.exclusive_scan(flags)
            assert total == flags.sum()
            wrong = scan_without_carry(flags)
            # caught wherever a flag is set in the first 256 tiles and one lies beyond them
            expect_caught = n > hp.SCAN_GROUP and flags[:hp.SCAN_GROUP].any()
            assert (wrong != right).any() == expect_caught, (n, name)
    big = hp.SCAN_SIZES[-1]
    assert big > 2 * hp.SCAN_GROUP + hp.SCAN_TILE and big % 8 != 0
    caught = [name for name in hp.FLAG_PATTERNS
              if (scan_without_carry(hp.flag_pattern(name, big))
                  != hp.exclusive_scan(hp.flag_pattern(name, big))[0]).any()]
    assert set(caught) == set(hp.FLAG_PATTERNS) - {"none", "last"}
    # the patterns are what their names say
    assert hp.flag_pattern("one_per_tile", 3 * 2048 + 5).reshape(-1)[:6144].reshape(3, 2048) \
        .sum(1).tolist() == [1, 1, 1]
    assert np.flatnonzero(hp.flag_pattern("tile_ends", 4097)).tolist() == [2047, 4095]
    assert hp.flag_pattern("none", 9).sum() == 0 and hp.flag_pattern("all", 9).sum() == 9


def means_with(case, skip_last=False, skip_lane=None):
    """f32(sum) / f32(count) of the integer kind with elements left out of the sum."""
    data, perm = case["data"], case["perm"]
    out = np.zeros((len(case["leaf_count"]), data.shape[1]), np.float32)
    for j, (start, count) in enumerate(zip(case["leaf_start"], case["leaf_count"])):
        rows = data[perm[start:start + count]].astype(np.float64)
        keep = np.ones(count, bool)
        if skip_last:
            keep[-1] = False
        if skip_lane is not None:
            keep[np.arange(count) % 64 == skip_lane] = False
        out[j] = np.float32(rows[keep].sum(0)) / np.float32(count)
    return out


def test_teeth_leaf_means():
    for name in hp.MEAN_CASES:
        case = hp.mean_case(name, "integers")
        right = hp.exact_means(case)
        assert np.isfinite(right).all() and right.dtype == np.float32
        assert means_with(case).tobytes() == right.tobytes()
        assert (case["perm"] != np.arange(len(case["perm"]))).any()
        assert (case["row_leaf"] < 0).any() and np.isnan(case["data"][case["row_leaf"] < 0]).all()
        # a mean that leaves out the last element is wrong in EVERY leaf and channel: the values
        # are >= 1 and the sums exact; one that leaves out lane 63 in every leaf of >= 64 points
        assert (means_with(case, skip_last=True) != right).all(), name
        lane = means_with(case, skip_lane=63) != right
        assert np.array_equal(lane.all(1), case["leaf_count"] >= 64), name
        assert np.array_equal(lane.any(1), case["leaf_count"] >= 64), name
    counts = set(sum((c for c, _ in hp.MEAN_CASES.values()), []))
    assert counts >= {1, 2, 63, 64, 65, 127, 128, 129, 4096, 4097, 1 << 20}
    assert {len(c) for c, _ in hp.MEAN_CASES.values()} >= {1, 3, 4, 5, 1025}
    assert {ch for _, ch in hp.MEAN_CASES.values()} == {1, 3, 4, 7}


def test_teeth_surface_points():
    """A fused multiply-add (one rounding) instead of product and sum (two) changes the bits of
    at least a quarter of the rows."""
    n = 4097
    inp = hp.surface_inputs(n)
    alpha = np.ones(n, np.float32)
    right, _ = oref.surface_points(alpha, inp["depth"], inp["starts"], inp["directions"], None,
                                   hp.THRESHOLD)
    fused = (inp["directions"].astype(np.float64) * inp["depth"].astype(np.float64)[:, None]
             + inp["starts"].astype(np.float64)).astype(np.float32)
    differ = (fused.view(np.uint32) != right.view(np.uint32)).any(1)
    print("rows an fma changes: %.3f" % differ.mean())
    assert differ.mean() >= 0.25
    assert np.array_equal(inp["starts"][:, 0], np.arange(n))
