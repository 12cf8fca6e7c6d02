"""Deep, SPARSE trees for the tests that hold the octree kernels at their depth limits (CPU and
GPU; nothing here needs a GPU).  A shallow hand-built tree (tests/octree_lattice_helpers.py,
tests/octree_mesh_cases.py) is embedded under one cell of a deeper tree: a few hundred leaves reach
depth 11, the limit of the walk family, or depth 21, the limit of K30, where leaf ids and corner
keys pass 2^31 and run up to 2^60."""

from collections import namedtuple
from functools import lru_cache

import numpy as np

from tests.octree_lattice_helpers import cell_id, grid_tree, lattice_rays, mixed_tree
from tests.octree_mesh_reference import leaf_levels_cells

DEEP11_AT = (37, 5, 62)             # the level-6 cell that holds ``mixed_tree()`` in ``deep11()``
DEEP11_LEVEL = 6
DEEP11_COARSE = ((1, 0, 0, 0), (2, 3, 3, 0), (3, 0, 7, 7), (4, 15, 0, 15), (5, 0, 31, 0))
DEEP11_SCALES = (2.0, 1.7)          # a power of two for the exact cases, and one that is not


def embed(leaf_index, leaf_level0, at, extra=()):
    """The leaves of a shallow tree under the cell ``at = (x, y, z)`` of level ``leaf_level0`` of a
    deeper tree: leaf ``(l, x, y, z)`` becomes ``(leaf_level0 + l, (at_x << l) + x, ...)``.
    ``extra``: further ``(level, x, y, z)`` leaves of the deep tree, outside that cell.
    -> node_index, leaf_index of the deep tree (``grid_tree``) and ``slots``: per shallow leaf, in
    the shallow order, its place among the deep tree's sorted leaves.  The embedded leaves keep
    their order (a deeper leaf has the larger id, and within a level the path code grows with the
    shallow one), so per-leaf data carries over unchanged: asserted."""
    leaf_index = np.asarray(leaf_index, np.int64)
    levels, cells = leaf_levels_cells(leaf_index)
    depth = leaf_level0 + int(levels.max()) + 1
    codes = [(leaf_level0 + l, (int(at[0]) << l) + x, (int(at[1]) << l) + y, (int(at[2]) << l) + z)
             for l, (x, y, z) in zip(levels.tolist(), cells.tolist())]
    depth = max([depth] + [int(c[0]) + 1 for c in extra])
    nodes, leaves = grid_tree(depth, codes + [tuple(int(v) for v in c) for c in extra])
    ids = np.array([cell_id(*c) for c in codes], np.int64)
    assert (np.diff(ids) > 0).all(), "the embedded leaves lost the shallow order"
    slots = np.searchsorted(leaves, ids)
    assert np.array_equal(leaves[slots], ids) and len(leaves) == len(codes) + len(extra)
    return nodes, leaves, slots


def cell_box(scale, at, level):
    """-> centre (3,) and half side, float64, of cell ``at`` of the 2^level grid of the cube
    ``+-scale``.  Exact for a power-of-two scale."""
    half = float(np.float32(scale)) / (1 << level)
    return -float(np.float32(scale)) + (np.asarray(at, np.float64) + 0.5) * 2.0 * half, half


@lru_cache(maxsize=None)
def deep11():
    """The walk tree, depth 11: ``mixed_tree()`` (depth 5) under the level-6 cell ``DEEP11_AT`` and
    five coarse leaves of levels 1 to 5 elsewhere, so that a ray crosses level-1 and level-10
    regions in one walk.  -> node_index, leaf_index, slots (of the mixed leaves).  Do not write
    into them."""
    _, _, shallow = mixed_tree()
    nodes, leaves, slots = embed(shallow, DEEP11_LEVEL, DEEP11_AT, DEEP11_COARSE)
    assert int(leaf_levels_cells(leaves[-1:])[0][0]) == 10
    return nodes, leaves, slots


def aimed_rays(scale, at, level, count, seed):
    """Rays aimed at the embedded cell: eyes on a sphere of radius 1.5 to 2.5 scales, targets
    uniform in cell ``at`` of ``level`` grown by 10 % a side, directions of unit length.
    -> starts, directions (count,3) f32."""
    rng = np.random.default_rng(seed)
    centre, half = cell_box(scale, at, level)
    eyes = rng.normal(size=(count, 3))
    eyes = eyes / np.linalg.norm(eyes, axis=1, keepdims=True) * rng.uniform(1.5, 2.5, (count, 1))
    o = eyes * float(np.float32(scale))
    target = centre + (rng.random((count, 3)) * 2 - 1) * half * 1.1
    d = target - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o.astype(np.float32), d.astype(np.float32)


def local_lattice_rays(scale, at, level, depth, count, seed):
    """The rays of ``lattice_rays(scale / 2^level, depth, ...)`` -- the lattice of a tree of
    ``depth`` that fills cell ``at`` of ``level`` -- with that cell's centre added to their starts.
    The centre is a multiple of the finest side of the tree of depth ``level + depth``, so the
    starts land on the lattice of its finest cells round that cell, with the same tie classes;
    directions stay in {0, +-0.5, +-1, +-2}."""
    starts, directions = lattice_rays(float(scale) / (1 << level), depth, count, seed)
    centre, _ = cell_box(scale, at, level)
    moved = (starts.astype(np.float64) + centre).astype(np.float32)
    assert np.array_equal(moved.astype(np.float64), starts.astype(np.float64) + centre)
    return moved, directions


# ------------------------------------------------------------------------- K30 at depth
MESH_DEPTHS = (11, 12, 16, 21)
MESH_NAMES = ("levels", "mixed", "random_sh2", "lone_coarse")
MESH_PLACES = ("zeros", "ones", "centre")
ZERO_LEAF = (1, 1, 0, 0)            # a level-1 leaf of density 0: 2^(D-2) finest cells a side
MASKED_LEAF = (1, 0, 1, 0)          # a level-1 leaf that only a caller's ``solid`` entry empties

DeepMesh = namedtuple("DeepMesh", "name depth scale nodes leaves leaf_data sh_degree slots at "
                                  "level0 shift solid")


@lru_cache(maxsize=None)
def deep_mesh(name, depth, place, masked=False) -> "DeepMesh":
    """``octree_mesh_cases.case(name)`` (depth ``d``) under a cell of level ``depth - d`` of a tree
    of ``depth``: the all-zero corner, the all-ones corner (the largest ids and keys, vertices at
    coordinate ``n`` on the cube's + faces) or the cell ``n'/2 - 1`` on each axis, whose vertices
    straddle the cube's centre.  ``scale = case.scale * 2^(depth - d)``: the finest side, and with
    it every opacity, keeps the shallow case's bits.

    Every tree also gets ``ZERO_LEAF``, a level-1 leaf of density 0, which has no candidates and
    leaves the mesh as it is.  ``masked``: the tree gets ``MASKED_LEAF`` too, with a density that
    WOULD make it solid, and ``solid`` (the shallow leaves' own solidity, False for both level-1
    leaves) is what a caller passes to keep it empty.

    NO SOLID LEAF HERE MAY HAVE MORE THAN 8^3 FINEST CELLS.  A solid leaf has ``6 k^2 + 2``
    candidates: a solid level-1 leaf at depth 21 would be ``6 * 2^38`` threads, a solid root
    ``6 * 2^40``.  A ``masked`` tree must therefore never be extracted without its ``solid``.

    ``shift``: what the embedding adds to a shallow corner, in finest cells."""
    from tests.octree_mesh_cases import case
    from tests import octree_mesh_reference as mref
    c = case(name)
    shallow_depth = mref.tree_depth(c.leaves)
    level0 = depth - shallow_depth
    assert level0 >= 2 and not c.kwargs
    cells = 1 << level0
    at = {"zeros": (0, 0, 0), "ones": (cells - 1,) * 3, "centre": (cells // 2 - 1,) * 3}[place]
    extra = (ZERO_LEAF, MASKED_LEAF) if masked else (ZERO_LEAF,)
    nodes, leaves, slots = embed(c.leaves, level0, at, extra)
    rows = np.zeros((len(leaves), c.leaf_data.shape[1]), c.leaf_data.dtype)
    rows[slots] = c.leaf_data
    solid = None
    if masked:
        where = np.searchsorted(leaves, cell_id(*MASKED_LEAF))
        rows[where, -1] = 50.0 / float(c.scale)         # opacity 1 over a finest side
        ref = mref.extract(c.scale, c.leaves, c.leaf_data, c.sh_degree)
        solid = np.zeros(len(leaves), bool)
        solid[slots] = ref.alpha > ref.threshold
    shift = np.asarray(at, np.int64) << (shallow_depth - 1)
    return DeepMesh(name, depth, float(c.scale) * 2.0 ** level0, nodes, leaves, rows, c.sh_degree,
                    slots, at, level0, shift, solid)


def f32_exact(w, starts, directions):
    """Is every crossing of the float64 walk ``w`` the same number in f32?  Redoes, per crossing
    and in f32, ``t = (plane - o) / d`` on the entry and the exit axis and the points
    ``o + t d``, and compares them with the float64 values.  -> bool."""
    o32, d32 = np.asarray(starts, np.float32), np.asarray(directions, np.float32)
    o, d = o32.astype(np.float64), d32.astype(np.float64)
    rows = np.arange(len(w["ray"]))
    ok = True
    for t, axis in ((w["t_in"], w["axis_in"]), (w["t_out"], w["axis_out"])):
        plane = o[w["ray"], axis] + t * d[w["ray"], axis]
        plane32 = plane.astype(np.float32)
        ok = ok and np.array_equal(plane32.astype(np.float64), plane)
        t32 = (plane32 - o32[w["ray"], axis]) / d32[w["ray"], axis]
        assert t32.dtype == np.float32
        ok = ok and np.array_equal(t32.astype(np.float64), t)
        product = t32[:, None] * d32[w["ray"]]
        point = o32[w["ray"]] + product
        assert point.dtype == np.float32 and len(rows) == len(point)
        ok = ok and np.array_equal(product.astype(np.float64), t[:, None] * d[w["ray"]])
        ok = ok and np.array_equal(point.astype(np.float64), o[w["ray"]] + t[:, None] * d[w["ray"]])
    return bool(ok)


# ------------------------------------------------------------------- the walk family at depth 11
WALK_RAYS = 4096
LEFT_OUT_CAP = 0.06         # of the aimed rays; depth-11 cells are 2e-3 scales wide (2 % at depth 6)
LATTICE_CASES = ("local lattice", "cube lattice")
AIMED_CASES = ("aimed 2.0", "aimed 1.7")


LATTICE_T_MINS = {"local lattice": (0.0, 2.0 ** -6), "cube lattice": (0.0, 1.25)}
# Optical depth of the lattice volume cases, as a multiple of ``random_leaf_data``'s: the rays of the
# whole-cube lattice mostly meet one coarse leaf, and end with 0.05 < T < 0.95 on 9 % of the rays
# that take a leaf at gain 1, on 73 % (t_min 0) and 61 % (t_min 1.25) at gain 32; the local lattice
# has 76 % and 63 % at gain 1.  From the restatement alone (``check_volume`` asserts 30 %).
LATTICE_DENSITY_GAIN = {"local lattice": 1.0, "cube lattice": 32.0}


def t_mins(name):
    """The two t_min of a walk case: 0, and a t that lies inside leaves on many rays -- for the
    aimed rays (eyes 1.5 to 2.5 scales from the cell) f32(1.5 scale)."""
    if name in LATTICE_T_MINS:
        return LATTICE_T_MINS[name]
    assert name in AIMED_CASES
    return (0.0, float(np.float32(1.5 * float(np.float32(float(name.split()[1]))))))


def lattice_data(name):
    """The leaf rows of a lattice case with its density gain.  Do not write into them."""
    data = walk_case(name)["data"].copy()
    data[:, 3] *= np.float32(LATTICE_DENSITY_GAIN[name])
    return data


def special_rays(scale, exact):
    """Two rays: one along the cube's main diagonal, through the coarse leaf (1, 0, 0, 0) and the
    large empty regions (the most descents per stop), and one along x through the embedded cell
    (the fewest).  ``exact``: from the cube's - corner through cell corners all the way, and
    through the centres of finest cells; otherwise a little off both, so that the margin rule
    keeps them."""
    s = float(np.float32(scale))
    centre, half = cell_box(scale, DEEP11_AT, DEEP11_LEVEL)
    if exact:
        fine = s / (1 << 10)                        # half a finest side
        starts = [[-s, -s, -s], [-s - 4 * fine, centre[1] + fine, centre[2] - 3 * fine]]
        dirs = [[1, 1, 1], [2, 0, 0]]
    else:
        starts = [[-1.5 * s, -1.52 * s, -1.47 * s],
                  [-2 * s, centre[1] + 0.31 * half, centre[2] - 0.77 * half]]
        dirs = [[3 ** -0.5] * 3, [1, 0, 0]]
    return np.float32(starts), np.float32(dirs)


@lru_cache(maxsize=None)
def walk_case(name):
    """-> dict, as ``case`` of tests/test_octree_lattice_gpu.py: ``deep11()`` with seeded leaf data,
    the rays of ``name`` (4096 and the two ``special_rays``) and their float64 walk ``w``.
    ``length``: a path length that cuts no ray, even with a zero-length stop before and after
    every region."""
    from tests import octree_walk_reference as wref
    from tests.octree_volume_helpers import random_leaf_data
    nodes, leaves, slots = deep11()
    if name == "local lattice":
        scale = 2.0
        starts, dirs = local_lattice_rays(scale, DEEP11_AT, DEEP11_LEVEL, 5, WALK_RAYS, 31)
    elif name == "cube lattice":
        scale = 2.0
        starts, dirs = lattice_rays(scale, 11, WALK_RAYS, 32)
    else:
        scale = float(name.split()[1])
        assert name in AIMED_CASES and scale in DEEP11_SCALES
        starts, dirs = aimed_rays(scale, DEEP11_AT, DEEP11_LEVEL, WALK_RAYS, 3)
    extra_s, extra_d = special_rays(scale, name in LATTICE_CASES)
    starts, dirs = np.concatenate([starts, extra_s]), np.concatenate([dirs, extra_d])
    w = wref.walk(scale, nodes, leaves, starts, dirs)
    longest = int(np.diff(w["offsets"]).max())
    return dict(name=name, scale=np.float32(scale), nodes=nodes, leaves=leaves, depth=11,
                data=random_leaf_data(scale, leaves), starts=starts, dirs=dirs, w=w,
                length=3 * longest + 2, slots=slots)


def left_out_share(c, t_min=None):
    """The share of the rays of ``walk_case`` ``c`` that the margin rule leaves out, by the float64
    walk and ``ray_budget`` alone; with ``t_min`` also the rays with a leaf that ends within the
    budget of it (the rule of the span, first-hit and volume tests)."""
    from tests.octree_walk_helpers import ray_budget
    w = c["w"]
    budget = ray_budget(w, c["scale"], c["starts"], c["dirs"])
    ok = ~w["hit"] | (w["margin"] > budget)
    if t_min is not None:
        close = (w["leaf"] >= 0) & (np.abs(w["t_out"] - t_min) <= budget[w["ray"]])
        near = np.zeros(len(ok), bool)
        near[w["ray"][close]] = True
        ok &= ~near
    return 1.0 - ok.mean()


# ------------------------------------------------- focus samples and visibility at depth 11
FOCUS_CASES = AIMED_CASES + LATTICE_CASES


@lru_cache(maxsize=None)
def focus_scene(name):
    """``walk_case(name)`` as a scene of tests/octree_focus_helpers.py: all its rays in WORLD space
    (a cube centre is added; one that keeps the lattice starts exact), with a ``[near, far]`` per
    ray: every fourth ``far`` ends inside or before the embedded cell, every ninth ``near`` begins
    late.  -> scene dict, its float64 walk and its restatement."""
    from tests import octree_focus_reference as fref
    from tests import octree_walk_reference as wref
    from tests.octree_focus_helpers import leaf_rows
    c = walk_case(name)
    f32 = np.float32
    count, scale = len(c["starts"]), float(c["scale"])
    if name in AIMED_CASES:
        center = f32([0.375, -1.25, 2.0])
        near, far = np.zeros(count, f32), np.full(count, 4 * scale, f32)
        far[::4], near[2::9] = f32(1.7 * scale), f32(1.5 * scale)
    elif name == "local lattice":
        center = f32([0.5, -1.0, 2.0])
        near, far = np.zeros(count, f32), np.full(count, 0.25, f32)
        far[::4], near[2::9] = f32(2.0 ** -6), f32(2.0 ** -7)
    else:
        center = f32([0.5, -1.0, 2.0])
        near, far = np.zeros(count, f32), np.full(count, 16, f32)
        far[::4], near[2::9] = f32(2.5), f32(0.75)
    world = (c["starts"] + center[None, :]).astype(f32)
    s = dict(name=name, scale=scale, depth=11, node_index=c["nodes"], leaf_index=c["leaves"],
             rows=leaf_rows(c["scale"], c["leaves"], 28), center=center, starts=world,
             directions=c["dirs"], near=near, far=far)
    back = (world - center[None, :]).astype(f32)                        # the kernel's subtraction
    if name in LATTICE_CASES:
        assert np.array_equal(back, c["starts"])
    w = wref.walk(scale, s["node_index"], s["leaf_index"], back, c["dirs"])
    return s, w, fref.cdf(w, scale, back, c["dirs"], near, far, s["rows"][:, 3])


def cell_cameras(scale, eyes, distance, width=24, height=20, fov_deg=14.0, look_at=None):
    """Cameras that look at ``look_at`` (the centre of the embedded cell of ``deep11()`` by default)
    from ``distance`` (in scales) along ``eyes``: ``look_at_camera`` moved from the origin to that
    point."""
    import fourier_feature_nets as ffn
    from tests.helpers import look_at_camera
    centre = cell_box(scale, DEEP11_AT, DEEP11_LEVEL)[0] if look_at is None else \
        np.asarray(look_at, np.float64)
    cameras = []
    for k, eye in enumerate(eyes):
        eye = np.asarray(eye, np.float64)
        intr, pose = look_at_camera(eye * distance * float(scale) / np.linalg.norm(eye), width,
                                    height, fov_deg)
        pose = np.array(pose, np.float64)
        pose[:3, 3] += centre
        cameras.append(ffn.CameraInfo.create("c%d" % k, ffn.Resolution(width, height), intr,
                                             pose.astype(np.float32)))
    return cameras


VISIBLE_EYES = ((-1.0, 0.3, -0.2), (0.4, 1.0, 0.3), (-0.3, -0.2, -1.0))   # into the cube


# ------------------------------------------- the grid builders at the top of the depth-11 codes
TOP_COUNT = 1000                                    # no multiple of a block
TOP_FIRST = 8 ** 10 - TOP_COUNT                     # the last codes: the largest is 2^30 - 1
TOP_CENTER = (0.1, 0.0, -0.1)
TOP_SCALE = 1.7
TOP_EYES = ((1.0, 0.6, 0.8), (0.7, 1.0, 0.5), (0.6, 0.8, 1.0))        # from outside the + corner


@lru_cache(maxsize=None)
def top_scene(fill=0.6, seed=7):
    """Three cameras of 24 x 20 that look at the cube's + corner from outside, so close that the
    last 1000 finest cells of a depth-11 grid (16 cells of 3.3e-3 a side) spread over the
    images; seeded RGBA (tests/carve_helpers.py) and the mask ``alpha >= 100``.
    -> images (3,20,24,4) u8, mask (3,20,24) u8, proj (3,3,4) f32."""
    import fourier_feature_nets as ffn
    from tests.carve_helpers import seeded_images
    corner = np.asarray(TOP_CENTER, np.float64) + TOP_SCALE
    inner = corner - 8 * 2 * TOP_SCALE / 1024       # the middle of those cells
    cameras = cell_cameras(TOP_SCALE, TOP_EYES, 0.25, fov_deg=9.0, look_at=inner)
    images = seeded_images(3, 20, 24, seed, fill)
    mask = (images[..., 3] >= 100).astype(np.uint8)
    return images, mask, ffn.projection_matrices(cameras)
