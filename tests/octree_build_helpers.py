"""Inputs made for the edges of the K12 build kernels (csrc/octree.hip), shared by
tests/test_octree_build_ops_cpu.py (which shows that they tell a subtly wrong kernel from a right
one) and tests/test_octree_build_ops_gpu.py (which runs the kernels on them).  numpy only.

The sizes come from the kernels' shapes: a flag scan tile is 2048 flags (256 threads x 8), one
workgroup scans the tile sums 256 at a time and carries between those groups (256 tiles = 524 288
flags); leaf_means gives one 64-lane wave to a leaf and four leaves to a workgroup."""

import numpy as np

SCAN_TILE = 2048
SCAN_GROUP = 256 * SCAN_TILE
SCAN_SIZES = [1, 7, 8, 9, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097,
              SCAN_GROUP - 1, SCAN_GROUP, SCAN_GROUP + 1, 2 * SCAN_GROUP + 2049 + 3]
FLAG_PATTERNS = ["all", "none", "first", "last", "alternating", "one_per_tile", "tile_ends",
                 "half", "sparse"]
MAX_DEPTH = 11


def flag_pattern(name, n):
    """-> (n,) bool."""
    flags = np.zeros(n, bool)
    if name == "all":
        flags[:] = True
    elif name == "first":
        flags[0] = True
    elif name == "last":
        flags[-1] = True
    elif name == "alternating":
        flags[1::2] = True
    elif name == "one_per_tile":            # somewhere else in every tile
        tiles = np.arange(0, n, SCAN_TILE)
        at = tiles + (tiles // SCAN_TILE * 37) % SCAN_TILE
        flags[at[at < n]] = True
    elif name == "tile_ends":               # the last flag of every tile
        flags[SCAN_TILE - 1::SCAN_TILE] = True
    elif name == "half":
        flags = np.random.default_rng(n).random(n) < 0.5
    elif name == "sparse":
        flags = np.random.default_rng(n + 1).random(n) < 0.01
    else:
        assert name == "none", name
    return flags


def exclusive_scan(flags):
    """What K12b/c computes: the number of set flags before each one, and their total."""
    flags = np.asarray(flags, bool)
    inclusive = np.cumsum(flags, dtype=np.int64)
    return inclusive - flags, int(inclusive[-1]) if len(flags) else 0


# ------------------------------------------------------------------------- surface points
THRESHOLD = 0.5


def surface_inputs(n, channels=4):
    """Rays whose rows say where they came from: ``starts[i, 0]`` is i (exact in f32 for
    n < 2^24) and ``color[i, 0]`` is i too, so a row written to the wrong place or taken from the
    wrong ray shows.  The y and z components are of order one on both sides of the sum, where
    ``fma(d, t, s)`` and ``round(round(d t) + s)`` differ for a good part of all inputs."""
    assert n < 1 << 24
    rng = np.random.default_rng(1000 + n)
    starts = (rng.random((n, 3), dtype=np.float32) * np.float32(4) - np.float32(2))
    starts[:, 0] = np.arange(n, dtype=np.float32)
    directions = rng.random((n, 3), dtype=np.float32) * np.float32(2) - np.float32(1)
    depth = rng.random(n, dtype=np.float32) * np.float32(3) + np.float32(0.5)
    color = rng.random((n, channels), dtype=np.float32)
    color[:, 0] = np.arange(n, dtype=np.float32)
    return dict(starts=starts, directions=directions, depth=depth, color=color)


def alpha_from_flags(flags):
    """alpha above the threshold where the flag is set; below it elsewhere, and for every third
    unset ray EXACTLY the threshold: '>' is strict, such a ray is not kept."""
    alpha = np.where(flags, np.float32(0.75), np.float32(0.25)).astype(np.float32)
    unset = np.flatnonzero(~flags)
    alpha[unset[::3]] = np.float32(THRESHOLD)
    return alpha


# ----------------------------------------------------------------------------- path codes
CUBES = [((0.3, -0.2, 0.1), 0.7), ((0.0, 0.0, 0.0), 1.0)]


def _step(x, toward):
    return np.nextafter(x, np.float32(toward)).astype(np.float32)


def path_code_positions(center, scale):
    """Positions (N,3) f32 around the cube ``center +- scale``: every lattice point
    ``center + scale k / 16`` (which holds the lattices of 2, 4 and 8 too: the splitting planes
    of four levels, the faces and the corners), each one f32 step down and up, positions
    outside on each side, positions on each face, NaN / +-inf / -0.0 coordinates, 10 000 random
    ones.  With the centre (0.3, -0.2, 0.1) the subtraction of the centre rounds."""
    f32 = np.float32
    c = np.asarray(center, f32)
    s = f32(scale)
    rng = np.random.default_rng(77)
    k = np.arange(-16, 17, dtype=f32) / f32(16)
    lattice = np.stack(np.meshgrid(k, k, k, indexing="ij"), -1).reshape(-1, 3)
    lattice = (c + s * lattice).astype(f32)
    parts = [lattice, _step(lattice, -np.inf), _step(lattice, np.inf)]
    inside = lambda m: (c + s * (rng.random((m, 3), dtype=f32) * f32(2) - f32(1))).astype(f32)
    for axis in range(3):
        for sign in (-1, 1):
            far = inside(50)
            far[:, axis] = c[axis] + f32(sign) * s * (f32(1) + rng.random(50, dtype=f32))
            face = inside(50)
            face[:, axis] = c[axis] + f32(sign) * s
            parts += [far, face]
    special = []
    for value in (np.nan, np.inf, -np.inf, -0.0, 0.0):
        for axis in range(3):
            p = inside(4)
            p[:, axis] = value
            special.append(p)
        special.append(np.full((1, 3), value, f32))
    parts += [np.concatenate(special), (c + s * f32(1.2) * (rng.random((10000, 3), dtype=f32)
                                                          * f32(2) - f32(1))).astype(f32)]
    return np.concatenate(parts).astype(f32)


# ------------------------------------------------------------------------------ structure
def node_id(*digits):
    """The id of the node reached from the root by these child indices."""
    node = 0
    for d in digits:
        node = 8 * node + 1 + d
    return node


def code_of(*digits):
    code = 0
    for d in digits:
        code = code * 8 + d
    return code


def structure_cases():
    """name -> dict(codes (sorted), depth, min_leaf_size, leaf (expected leaf id per sorted point),
    leaves (expected (id, start, count) rows in code order)).  The answers are written out here by
    hand from octree.py:762-803; nothing computes them."""
    c = code_of
    cases = {}

    def add(name, codes, depth, min_leaf, leaf, leaves):
        cases[name] = dict(codes=np.asarray(codes, np.int64), depth=depth, min_leaf_size=min_leaf,
                           leaf=np.asarray(leaf, np.int64),
                           leaves=np.asarray(leaves, np.int64).reshape(-1, 3))

    # child 0 of the root holds 3 points and is followed; its seven siblings hold one each
    add("starved_siblings_depth2", [0, 0, 0, 1, 2, 3, 4, 5, 6, 7], 2, 3,
        [1, 1, 1] + [-1] * 7, [(1, 0, 3)])
    # the same one level down: within node 1, child 0 (2 points) is followed, child 1 starves
    add("starved_siblings_depth3",
        [c(0, 0), c(0, 0), c(0, 1)] + [c(j, 0) for j in range(1, 8)], 3, 2,
        [9, 9, -1] + [-1] * 7, [(9, 0, 2)])
    # node 1 is followed (3 points) but none of its children is: node 1 is a leaf with all three;
    # the point in node 2 is dropped
    add("no_followed_child", [c(0, 0), c(0, 1), c(0, 2), c(1, 0)], 3, 3,
        [1, 1, 1, -1], [(1, 0, 3)])
    # no child of the root is followed: the root is the leaf
    add("root_is_the_leaf", [c(0, 0), c(1, 1), c(2, 2), c(3, 3)], 3, 2,
        [0, 0, 0, 0], [(0, 0, 4)])
    # a chain followed to level D - 1 = 10, next to a point that leaves it at the last level
    deep = (1, 2, 3, 4, 5, 6, 7, 0, 1, 2)
    add("chain_to_the_last_level", [c(*deep), c(*deep), c(*deep[:-1], 3)], 11, 2,
        [node_id(*deep), node_id(*deep), -1], [(node_id(*deep), 0, 2)])
    # four points in child 3 of the root, two in each of its children 0 and 1
    four = [c(3, 0), c(3, 0), c(3, 1), c(3, 1)]
    # exactly n: node 4 is followed (4 >= 4), its children are not: node 4 holds all four
    add("min_leaf_is_n", four, 3, 4, [4] * 4, [(4, 0, 4)])
    # above n and depth > 1: the root is still visited and has no child to follow, so it is the
    # leaf (octree.py:793-801); only at depth 1 does such a cloud give no leaf at all
    add("min_leaf_is_n_plus_1", four, 3, 5, [0] * 4, [(0, 0, 4)])
    add("min_leaf_is_1", four, 3, 1, [33, 33, 34, 34], [(33, 0, 2), (34, 2, 2)])
    add("min_leaf_above_n_at_depth_1", four, 1, 5, [-1] * 4, [])
    add("min_leaf_is_n_at_depth_1", four, 1, 4, [0] * 4, [(0, 0, 4)])
    for n in (1, 2047, 2048, 2049):
        add("all_codes_equal_%d" % n, [c(7, 3, 5)] * n, 4, 1, [node_id(7, 3, 5)] * n,
            [(node_id(7, 3, 5), 0, n)])
    # every path of four levels once: 4096 leaves of one point, ids 585 .. 4680 in code order
    every = np.arange(4096)
    add("every_code_of_four_levels", every, 5, 1, 585 + every,
        np.stack([585 + every, every, np.ones(4096, np.int64)], 1))
    # the largest code: all 30 bits set; its leaf is the last id of level 10
    top = 8 ** 10 - 1
    add("largest_code", [0, top], 11, 1, [153391689, 153391689 + top],
        [(153391689, 0, 1), (153391689 + top, 1, 1)])
    return cases


def scramble(n, seed=5):
    """A permutation of [0, n) that is not the identity for n > 1."""
    perm = np.random.default_rng(seed).permutation(n)
    if n > 1 and (perm == np.arange(n)).all():
        perm = perm[::-1].copy()
    return perm.astype(np.int64)


# ----------------------------------------------------------------------------- leaf means
WAVE_COUNTS = [1, 2, 63, 64, 65, 127, 128, 129]
MEAN_CASES = {
    # name: (leaf counts, channels)
    "wave_edges": (WAVE_COUNTS + [4096, 4097], 3),
    "one_leaf_of_2^20": ([1 << 20], 1),
    "three_leaves": ([64, 65, 63], 4),
    "four_leaves": ([129, 1, 128, 2], 4),
    "five_leaves": ([65, 64, 127, 2, 63], 7),
    "1025_leaves": ([WAVE_COUNTS[i % 8] for i in range(1025)], 3),
}


def mean_case(name, kind, outsider=np.nan):
    """-> dict(data (N,C) f32 in the CALLER's row order, perm (N,) int64 (sorted position -> row,
    not the identity), leaf_start / leaf_count per leaf into perm, row_leaf (N,): the leaf of
    every row or -1).  Between the leaves, and before the first, lie one to three rows that belong
    to no leaf; their data is ``outsider``.  kind "integers": values 1 .. 15, every partial sum
    of a leaf stays below 2^24 and is exact in f32 in any order; kind "random": uniform f32."""
    counts, channels = MEAN_CASES[name]
    rng = np.random.default_rng(len(counts) * 31 + channels)
    gaps = rng.integers(1, 4, len(counts))
    start = np.cumsum(gaps + np.concatenate([[0], counts[:-1]])).astype(np.int64)
    n = int(start[-1] + counts[-1] + 2)
    sorted_leaf = np.full(n, -1, np.int64)
    for j, (s, k) in enumerate(zip(start, counts)):
        sorted_leaf[s:s + k] = j
    perm = scramble(n, seed=len(counts))
    if kind == "integers":
        assert max(counts) * 15 < 1 << 24
        values = rng.integers(1, 16, (n, channels)).astype(np.float32)
    else:
        values = rng.random((n, channels), dtype=np.float32) * np.float32(2) - np.float32(0.5)
    values[sorted_leaf < 0] = outsider
    data = np.empty_like(values)
    data[perm] = values                      # sorted position i holds row perm[i]
    row_leaf = np.empty(n, np.int64)
    row_leaf[perm] = sorted_leaf
    return dict(data=data, perm=perm, leaf_start=start, leaf_count=np.asarray(counts, np.int32),
                row_leaf=row_leaf)


def exact_means(case):
    """For the integer kind: f32(exact sum) / f32(count), one correctly rounded f32 division."""
    counts = case["leaf_count"]
    keep = case["row_leaf"] >= 0
    sums = np.zeros((len(counts), case["data"].shape[1]), np.int64)
    np.add.at(sums, case["row_leaf"][keep], case["data"][keep].astype(np.int64))
    assert sums.max() < 1 << 24
    return sums.astype(np.float32) / counts.astype(np.float32)[:, None]


# -------------------------------------------------------------------------------- queries
def chain_query_positions(scale, count=100000):
    """Positions for a tree of scale ``scale``: a quarter on the faces, a quarter outside, a
    quarter dyadic multiples of the scale (splitting planes of up to 20 levels), the rest
    random."""
    f32 = np.float32
    scale = f32(scale)
    rng = np.random.default_rng(4242)
    quarter = count // 4
    q = (rng.random((count, 3), dtype=f32) * f32(2) - f32(1)) * scale
    rows = np.arange(quarter)
    q[rows, rng.integers(0, 3, quarter)] = scale * rng.choice(f32([-1, 1]), quarter)
    rows = np.arange(quarter, 2 * quarter)
    q[rows, rng.integers(0, 3, quarter)] = (scale * (f32(1) + rng.random(quarter, dtype=f32))
                                            * rng.choice(f32([-1, 1]), quarter))
    q[rows[0]] = np.nextafter(scale, f32(np.inf))         # one step outside on every axis
    power = rng.integers(1, 21, size=(quarter, 1))
    k = rng.integers(-(2 ** power), 2 ** power + 1, size=(quarter, 3))
    q[2 * quarter:3 * quarter] = (k / 2.0 ** power).astype(f32) * scale
    return q.astype(f32)
