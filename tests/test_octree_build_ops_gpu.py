"""The K12 octree build kernels (csrc/octree.hip) one op at a time, through ``ops.*``, on the
inputs of tests/octree_build_helpers.py: the flag scan at its tile (2048) and carry (256 tiles)
edges under chosen flag patterns, path codes for a caller's cube at every depth 1 .. 11, the
sibling rule of ``assign`` on hand cases with written-out answers, interior nodes, leaf means at
the wave and workgroup edges, ``query`` / ``leaf_geometry`` on the deepest tree an int64 id allows,
whole builds of the degenerate clouds the reference built (tests/golden/octree_edges.npz).

Every comparison is EQUALITY of integers or of f32 bit patterns against tests/octree_reference.py
or the reference's own record, except the means of random data, held to ``mean_bound`` of
tests/test_octree_cpu.py.  tests/test_octree_build_ops_cpu.py shows that these inputs change the
answer of a restatement that is wrong in the ways a kernel could be.

The means of integer data (exact sums) are held to ``f32(sum) / f32(count)`` bit for bit at every
count: the library is built without fast-math and the compiler's default f32 division is correctly
rounded.  On the MI355X this holds at the counts that are no power of two as well; the test prints
how many means differ before it asserts."""

import numpy as np
import pytest
import torch

from tests import octree_build_helpers as hp
from tests import octree_reference as oref
from tests.test_octree_build_ops_cpu import ALL_CLOUDS, EDGE_CLOUDS, cloud, load, rebuilt
from tests.test_octree_cpu import mean_bound

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def gpu(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(dtype)).to(dev())


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def golden():
    return {"octree.npz": load("octree.npz"), "octree_edges.npz": load("octree_edges.npz")}


@pytest.fixture(scope="module")
def ops():
    from fourier_feature_nets_amd import ops
    return ops


# ------------------------------------------------------------------- scan and surface points
@pytest.mark.parametrize("n", hp.SCAN_SIZES)
def test_surface_points_under_every_flag_pattern(ops, n):
    """K12a-d: every flag pattern at this size; the channel count goes round 0, 1, 3, 4."""
    inp = hp.surface_inputs(n)
    dev_in = {k: gpu(v) for k, v in inp.items()}
    keep = {k: v.clone() for k, v in dev_in.items()}
    for at, name in enumerate(hp.FLAG_PATTERNS):
        channels = (0, 1, 3, 4)[at % 4]
        flags = hp.flag_pattern(name, n)
        alpha = hp.alpha_from_flags(flags)
        assert flags.all() or (alpha == np.float32(hp.THRESHOLD)).any()
        color = inp["color"][:, :channels] if channels else None
        dev_color = dev_in["color"][:, :channels].contiguous() if channels else None
        dev_alpha = gpu(alpha)
        pos, col, count = ops.octree_surface_points(dev_alpha, dev_in["depth"], dev_in["starts"],
                                                    dev_in["directions"], hp.THRESHOLD, dev_color)
        k = int(count.item())
        assert k == int(flags.sum()), (name, k)
        want_pos, want_col = oref.surface_points(alpha, inp["depth"], inp["starts"],
                                                 inp["directions"], color, hp.THRESHOLD)
        pos = pos.cpu().numpy()
        assert pos.shape == (n, 3) and np.array_equal(bits(pos[:k]), bits(want_pos)), name
        assert not bits(pos[k:]).any(), name               # rows past count: +0.0
        if channels:
            col = col.cpu().numpy()
            assert col.shape == (n, channels)
            assert np.array_equal(bits(col[:k]), bits(want_col)), name
            assert not bits(col[k:]).any(), name
        else:
            assert col is None
        # the wrapper allocates its outputs itself: the inputs are as they were
        assert torch.equal(dev_alpha, gpu(alpha))
        for key, value in keep.items():
            assert torch.equal(dev_in[key], value), (name, key)


# --------------------------------------------------------------------------------- path codes
@pytest.fixture(scope="module")
def code_inputs():
    out = []
    for center, scale in hp.CUBES:
        positions = hp.path_code_positions(center, scale)
        out.append((center, scale, positions, gpu(positions)))
    return out


@pytest.mark.parametrize("depth", list(range(1, hp.MAX_DEPTH + 1)))
def test_path_codes_for_a_callers_cube(ops, code_inputs, depth):
    for center, scale, positions, dev_positions in code_inputs:
        want = oref.path_codes(positions, center, scale, depth)
        got = ops.octree_path_codes(dev_positions, center, scale, depth)
        assert got.dtype == torch.int32 and got.shape == (len(positions),)
        got = got.cpu().numpy().astype(np.int64)
        wrong = np.flatnonzero(got != want)
        assert len(wrong) == 0, (center, positions[wrong[:5]], got[wrong[:5]], want[wrong[:5]])
        for n in (1, 257):                      # one thread; one thread of a second workgroup
            few = ops.octree_path_codes(dev_positions[-n:].contiguous(), center, scale, depth)
            assert np.array_equal(few.cpu().numpy(), want[-n:])
    if depth == hp.MAX_DEPTH:
        assert want.max() == 8 ** 10 - 1        # all 30 bits


# ---------------------------------------------------------------------------------- structure
def run_structure(ops, codes, depth, min_leaf, perm):
    """-> leaf per point in the CALLER's order (numpy), (id, start, count) rows in code order."""
    point_leaf, ids, start, count = ops.octree_structure(gpu(codes, torch.int32), gpu(perm), depth,
                                                         min_leaf)
    assert point_leaf.dtype == torch.int64 and ids.dtype == torch.int64
    assert start.dtype == torch.int64 and count.dtype == torch.int32
    rows = np.stack([ids.cpu().numpy(), start.cpu().numpy(),
                     count.cpu().numpy().astype(np.int64)], 1).reshape(-1, 3)
    return point_leaf.cpu().numpy(), rows


@pytest.mark.parametrize("name", sorted(hp.structure_cases()))
def test_structure_hand_cases(ops, name):
    case = hp.structure_cases()[name]
    n = len(case["codes"])
    perm = hp.scramble(n)
    point_leaf, rows = run_structure(ops, case["codes"], case["depth"], case["min_leaf_size"], perm)
    want = np.empty(n, np.int64)
    want[perm] = case["leaf"]                   # sorted position i is the caller's point perm[i]
    assert np.array_equal(point_leaf, want)
    assert np.array_equal(rows, case["leaves"])


@pytest.mark.parametrize("file,name", ALL_CLOUDS)
def test_structure_and_interior_nodes_of_the_fixture_clouds(ops, golden, file, name):
    c = cloud(golden[file], name)
    mine = rebuilt(c)
    depth, min_leaf = int(c["depth"]), int(c["min_leaf_size"])
    point_leaf, rows = run_structure(ops, mine["codes"][mine["perm"]], depth, min_leaf, mine["perm"])
    assert np.array_equal(point_leaf, mine["point_leaf"])
    assert np.array_equal(rows, mine["leaves"])
    nodes = ops.octree_interior_nodes(gpu(rows[:, 0]), depth).cpu().numpy()
    check_nodes(nodes, rows[:, 0])
    assert np.array_equal(np.sort(nodes), c["node_index"])
    # and above every count: the root holds everything at depth > 1, nothing is left at depth 1
    point_leaf, rows = run_structure(ops, mine["codes"][mine["perm"]], depth, len(mine["codes"]) + 1,
                                     mine["perm"])
    if depth == 1:
        assert len(rows) == 0 and (point_leaf == -1).all()
    else:
        assert np.array_equal(rows, [[0, 0, len(point_leaf)]]) and (point_leaf == 0).all()


def test_min_leaf_size_above_n_at_depth_1_gives_no_leaf(ops):
    for n in (1, 5, 2049):
        point_leaf, rows = run_structure(ops, np.zeros(n, np.int64), 1, n + 1, hp.scramble(n))
        assert rows.shape == (0, 3) and (point_leaf == -1).all()


# ----------------------------------------------------------------------------- interior nodes
def check_nodes(nodes, leaf_ids):
    want = oref.interior_nodes(leaf_ids)
    assert len(np.unique(nodes)) == len(nodes), "an interior node twice"
    assert not np.isin(nodes, leaf_ids).any(), "a leaf among the interior nodes"
    assert np.array_equal(np.sort(nodes), want)


@pytest.mark.parametrize("name", sorted(hp.structure_cases()))
def test_interior_nodes_of_the_hand_cases(ops, name):
    case = hp.structure_cases()[name]
    ids = case["leaves"][:, 0]
    nodes = ops.octree_interior_nodes(gpu(ids), case["depth"])
    assert nodes.dtype == torch.int64
    if len(ids) == 0 or case["depth"] == 1:
        assert nodes.shape == (0,)
        return
    check_nodes(nodes.cpu().numpy(), ids)
    if case["depth"] < hp.MAX_DEPTH:            # a depth argument beyond the deepest leaf
        check_nodes(ops.octree_interior_nodes(gpu(ids), hp.MAX_DEPTH).cpu().numpy(), ids)


def test_interior_nodes_at_depth_2_and_at_mixed_depths(ops):
    every = np.arange(1, 9)
    for ids in (every, every[[0]], every[[7]], every[[2, 5]]):
        assert ops.octree_interior_nodes(gpu(ids), 2).cpu().numpy().tolist() == [0]
    nid = hp.node_id                            # leaves of levels 1, 3, 2, 10 and 1, in code order
    ids = np.array([nid(0), nid(1, 0, 0), nid(1, 0, 7), nid(1, 3), nid(1, 7, 7),
                    nid(5, *[4] * 9), nid(5, *[4] * 8, 5), nid(7)])
    check_nodes(ops.octree_interior_nodes(gpu(ids), 11).cpu().numpy(), ids)
    assert len(oref.interior_nodes(ids)) == 1 + 1 + 2 + 9


@pytest.mark.parametrize("depth,k", [(9, 255), (9, 256), (9, 257), (5, 511), (5, 512), (5, 513)])
def test_interior_nodes_at_the_scan_tile(ops, golden, depth, k):
    """k leaves x (depth - 1) levels of ancestor flags around the scan tile: 2040 / 2048 / 2056 at
    depth 9, 2044 / 2048 / 2052 at depth 5.  (No tree gives 2047 = 23 x 89 or 2049 = 3 x 683 flags:
    depth - 1 would be 1 or 3, and such a tree has at most 8 or 512 leaves.)  The leaves are the
    first k, in code order, of a real tree."""
    positions = cloud(golden["octree_edges.npz"], "depth11_min1")["positions"]
    mine = rebuilt(dict(positions=positions, depth=depth, min_leaf_size=1))
    assert len(mine["leaves"]) >= k
    ids = mine["leaves"][:k, 0]
    assert k * (depth - 1) in (2040, 2048, 2056, 2044, 2052)
    check_nodes(ops.octree_interior_nodes(gpu(ids), depth).cpu().numpy(), ids)


# --------------------------------------------------------------------------------- leaf means
def run_means(ops, case):
    out = ops.octree_leaf_means(gpu(case["data"]), gpu(case["perm"]), gpu(case["leaf_start"]),
                                gpu(case["leaf_count"]))
    assert out.dtype == torch.float32
    return out.cpu().numpy()


@pytest.mark.parametrize("name", sorted(hp.MEAN_CASES))
def test_leaf_means_of_integer_data_are_exact(ops, name):
    """Sums below 2^24 are exact in any order, so the mean is one f32 division: bits equal."""
    case = hp.mean_case(name, "integers")
    want = hp.exact_means(case)
    got = run_means(ops, case)
    assert got.shape == want.shape
    off = bits(got) != bits(want)
    print("leaf means %s: %d of %d differ from f32(sum) / f32(count)" % (name, off.sum(), off.size))
    assert np.isfinite(got).all()               # the rows of no leaf hold NaN
    assert not off.any(), (case["leaf_count"][off.any(1)][:8], got[off][:8], want[off][:8])
    assert bits(run_means(ops, case)).tobytes() == bits(got).tobytes()


@pytest.mark.parametrize("name", sorted(hp.MEAN_CASES))
def test_leaf_means_of_random_data_within_the_bound(ops, name):
    case = hp.mean_case(name, "random")
    got = run_means(ops, case)
    keep = case["row_leaf"] >= 0
    counts = case["leaf_count"].astype(np.int64)
    sums = np.zeros(got.shape, np.float64)
    np.add.at(sums, case["row_leaf"][keep], case["data"][keep].astype(np.float64))
    want = sums / counts[:, None]
    bound = mean_bound(np.nan_to_num(case["data"]), case["row_leaf"], np.arange(len(counts)), counts)
    err = np.abs(got.astype(np.float64) - want)
    print("leaf means %s: max err / bound = %.3f" % (name, (err / bound).max()))
    assert np.isfinite(got).all() and (err <= bound).all()
    assert bits(run_means(ops, case)).tobytes() == bits(got).tobytes()


# ------------------------------------------------------------------ query and leaf geometry
@pytest.fixture(scope="module")
def chain(golden):
    import fourier_feature_nets as ffn
    g = cloud(golden["octree_edges.npz"], "chain")
    tree = ffn.OcTree.load({"node_index": g["node_index"], "leaf_index": g["leaf_index"],
                            "scale": g["scale"]})
    return g, tree


def test_deep_chain_geometry_and_answers_equal_the_reference(chain):
    g, tree = chain
    assert tree.depth == 21 and tree.num_leaves == 141
    assert np.array_equal(bits(tree.leaf_centers()), bits(g["leaf_centers"]))
    assert tree.leaf_depths().dtype == np.int32
    assert np.array_equal(tree.leaf_depths(), g["leaf_depths"])
    answers = tree.query(g["query"])
    assert answers.dtype == np.int64 and np.array_equal(answers, g["query_result"])


def test_deep_chain_answers_equal_the_restatement(chain):
    g, tree = chain
    scale = g["scale"]
    q = hp.chain_query_positions(scale)
    # the deep end of the chain is small: crowd a part of the random quarter around its leaves
    rng = np.random.default_rng(6)
    pick = rng.integers(0, len(g["leaf_centers"]), 12000)
    spread = scale * np.float32(1.5) * np.float32(2.0) ** -g["leaf_depths"][pick, None].astype(np.float32)
    q[-12000:] = g["leaf_centers"][pick] + spread * (rng.random((12000, 3), dtype=np.float32) * 2 - 1)
    assert len(q) == 100000
    want = oref.query(scale, g["node_index"], g["leaf_index"], q)
    outside = (np.abs(q) > scale).any(1)
    assert outside.mean() > 0.2 and ((np.abs(q) == scale).any(1) & ~outside).sum() > 10000
    assert (want[outside] == -1).all()
    levels = g["leaf_depths"][want[want >= 0]]
    assert (levels == 20).sum() > 100 and len(np.unique(levels)) == 20
    assert np.array_equal(tree.query(q), want)


def test_walk_still_refuses_the_deep_chain(chain):
    _, tree = chain
    with pytest.raises(ValueError, match="deeper than the ray walk"):
        tree.walk(np.zeros((1, 3), np.float32), np.ones((1, 3), np.float32), 8)


# ------------------------------------------------------------------------------- whole builds
@pytest.mark.parametrize("name", EDGE_CLOUDS)
def test_edge_clouds_build_as_the_reference_built_them(golden, name):
    import fourier_feature_nets as ffn
    g = cloud(golden["octree_edges.npz"], name)
    before = g["positions"].copy()
    tree = ffn.OcTree.build_from_samples(g["positions"], int(g["depth"]), int(g["min_leaf_size"]),
                                         g.get("data"))
    assert np.array_equal(g["positions"], before)
    state = tree.state_dict
    assert np.array_equal(state["node_index"], g["node_index"])
    assert np.array_equal(state["leaf_index"], g["leaf_index"])
    assert np.float32(state["scale"]).tobytes() == g["scale"].tobytes()
    expect = oref.build(before, int(g["depth"]), int(g["min_leaf_size"]), g.get("data"))
    assert np.array_equal(tree.point_leaf_ids.cpu().numpy(), expect["point_leaf"])
    if "data" in g:
        got = tree.leaf_data()
        assert got.dtype == np.float32 and got.shape == g["leaf_data"].shape
        bound = mean_bound(g["data"], expect["point_leaf"], expect["leaf_index"],
                           expect["leaf_count"])
        assert (np.abs(got.astype(np.float64) - expect["leaf_data"]) <= bound).all()
    else:
        assert tree.leaf_data() is None
    if "leaf_centers" in g:
        assert np.array_equal(bits(tree.leaf_centers()), bits(g["leaf_centers"]))
        assert np.array_equal(tree.leaf_depths(), g["leaf_depths"])
        assert np.array_equal(tree.query(g["query"]), g["query_result"])
    else:
        assert name == "min_equals_n" and np.array_equal(tree.leaf_depths(), [0])
    if name == "identical":
        assert tree.scale == 0.0 and tree.num_leaves == 1 and tree.leaf_depths()[0] == 5
        assert not bits(tree.leaf_centers()).any()
        assert tree.query(np.zeros((1, 3), np.float32))[0] == 0
        assert tree.query(np.float32([[-0.0, 0.0, -0.0]]))[0] == 0
        tiny = np.nextafter(np.float32(0), np.float32(1))
        for axis in range(3):
            for step in (tiny, -tiny):
                p = np.zeros((1, 3), np.float32)
                p[0, axis] = step
                assert tree.query(p)[0] == -1


# --------------------------------------------------------------------------------- refusals
def test_empty_inputs_give_empty_outputs(ops):
    f = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev())
    i64 = lambda n: torch.zeros((n,), dtype=torch.int64, device=dev())
    pos, col, count = ops.octree_surface_points(f(0), f(0), f(0, 3), f(0, 3), 0.5, f(0, 3))
    assert pos.shape == (0, 3) and col.shape == (0, 3) and int(count.item()) == 0
    assert ops.octree_path_codes(f(0, 3), (0, 0, 0), 1.0, 5).shape == (0,)
    out = ops.octree_structure(i64(0).to(torch.int32), i64(0), 5, 1)
    assert [tuple(t.shape) for t in out] == [(0,)] * 4
    assert ops.octree_interior_nodes(i64(0), 5).shape == (0,)
    assert ops.octree_leaf_means(f(3, 2), i64(3), i64(0), i64(0).to(torch.int32)).shape == (0, 2)
    assert ops.octree_query(f(0, 3), 1.0, i64(1), i64(1) + 1).shape == (0,)
    centers, depths = ops.octree_leaf_geometry(i64(0), 1.0)
    assert centers.shape == (0, 3) and depths.shape == (0,)


def _refused(match, fn, *outs):
    from fourier_feature_nets_amd._lib import FfnError
    with pytest.raises(FfnError, match=match):
        fn()
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o == -7).all()), "%s: the refused call wrote its output" % match


def test_out_of_range_shapes_are_refused_before_any_launch(ops):
    from fourier_feature_nets_amd._lib import FfnError, c_f, c_i, c_i64
    n = 8
    sentinel = lambda dtype: torch.full((n,), -7, dtype=dtype, device=dev())
    positions = torch.zeros((n, 3), dtype=torch.float32, device=dev())
    codes32 = torch.zeros((n,), dtype=torch.int32, device=dev())
    perm = torch.arange(n, dtype=torch.int64, device=dev())
    flags = torch.zeros((n * 16,), dtype=torch.uint8, device=dev())
    offsets = torch.zeros((n * 16,), dtype=torch.int32, device=dev())
    tiles = torch.zeros((4,), dtype=torch.int32, device=dev())
    ids = torch.arange(1, n + 1, dtype=torch.int64, device=dev())
    d = ops._dev

    def path_codes(depth, positions=positions, out=None):
        return lambda: ops._call("ffn_octree_path_codes", d(positions), c_i64(n), c_f(0), c_f(0),
                                 c_f(0), c_f(1), c_i(depth), d(out, torch.int32))

    def structure(depth, out, codes=codes32):
        leaf_sorted, count_sorted, point_leaf, leaf_ids, start, count, num = out
        return lambda: ops._call(
            "ffn_octree_structure", d(codes, torch.int32), d(perm, torch.int64), c_i64(n),
            c_i(depth), c_i64(1), d(leaf_sorted, torch.int64), d(count_sorted, torch.int32),
            d(point_leaf, torch.int64), d(flags, torch.uint8), d(offsets, torch.int32),
            d(tiles, torch.int32), d(leaf_ids, torch.int64), d(start, torch.int64),
            d(count, torch.int32), d(num, torch.int32))

    def interior(depth, out, num, leaf_ids=ids):
        return lambda: ops._call("ffn_octree_interior_nodes", d(leaf_ids, torch.int64), c_i64(n),
                                 c_i(depth), d(flags, torch.uint8), d(offsets, torch.int32),
                                 d(tiles, torch.int32), d(out, torch.int64), d(num, torch.int32))

    def structure_outs():
        return [sentinel(t) for t in (torch.int64, torch.int32, torch.int64, torch.int64,
                                      torch.int64, torch.int32, torch.int32)]

    for depth in (0, hp.MAX_DEPTH + 1, -1):
        out = sentinel(torch.int32)
        _refused("1 <= depth <= 11", path_codes(depth, out=out), out)
        outs = structure_outs()
        _refused("1 <= depth <= 11", structure(depth, outs), *outs)
        out, num = sentinel(torch.int64), sentinel(torch.int32)
        _refused("2 <= depth <= 11", interior(depth, out, num), out, num)
        # the wrappers pass the refusal on
        with pytest.raises(FfnError, match="depth"):
            ops.octree_path_codes(positions, (0, 0, 0), 1.0, depth)
        with pytest.raises(FfnError, match="depth"):
            ops.octree_structure(codes32, perm, depth, 1)
    with pytest.raises(FfnError, match="depth"):
        ops.octree_interior_nodes(ids, hp.MAX_DEPTH + 1)
    # a null argument
    out = sentinel(torch.int32)
    _refused("null argument", path_codes(5, positions=None, out=out), out)
    _refused("null argument", path_codes(5, out=None))
    outs = structure_outs()
    _refused("null argument", structure(5, outs, codes=None), *outs)
    out, num = sentinel(torch.int64), sentinel(torch.int32)
    _refused("null argument", interior(5, out, num, leaf_ids=None), out, num)
    means = torch.full((2, 3), -7.0, device=dev())
    _refused("null argument", lambda: ops._call(
        "ffn_octree_leaf_means", d(None), c_i64(n), c_i(3), d(perm, torch.int64),
        d(perm, torch.int64), d(codes32, torch.int32), c_i64(2), d(means)), means)
    answers = sentinel(torch.int64)
    _refused("null argument", lambda: ops._call(
        "ffn_octree_query", d(positions), c_i64(n), c_f(1), d(None, torch.int64), c_i64(0),
        d(None, torch.int64), c_i64(1), d(answers, torch.int64)), answers)
    centers = torch.full((n, 3), -7.0, device=dev())
    _refused("null argument", lambda: ops._call(
        "ffn_octree_leaf_geometry", d(ids, torch.int64), c_i64(n), c_f(1), d(centers),
        d(None, torch.int32)), centers)
    # and the same call with everything in place goes through: the origin of the cube 0 +- 1 takes
    # child 7 of the root (0 >= 0), then child 0 of every node below (0 < 1/2, 1/4, 1/8)
    out = sentinel(torch.int32)
    path_codes(5, out=out)()
    assert bool((out == 0o7000).all())
