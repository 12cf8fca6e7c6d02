"""Scenes shared by the K26 tests (CPU and GPU): trees from the existing helpers at depth <= 6 and a
root-only tree, with a density per leaf, world-space rays with their ``[near, far]`` and a cube
centre.  The densities are chosen so that a ray's mass is either 0 or far above ``MIN_MASS`` (the
CPU test asserts that the restatement finds no undecided ray).  The float64 restatement of a scene
is made once and shared (``reference``)."""

import functools

import numpy as np

from tests import octree_focus_reference as fref
from tests import octree_reference as oref
from tests import octree_walk_reference as wref
from tests.octree_lattice_helpers import lattice_rays, mixed_tree
from tests.octree_render_helpers import camera_rays, golden_rays
from tests.octree_walk_helpers import two_level_tree

MIN_MASS = 1e-3
SCENES = ["hand", "root", "shell", "planes", "mixed"]


def leaf_rows(scale, leaf_index, seed):
    """(L,4) f32 rows [r, g, b, sigma]: an optical depth of 0.5 .. 1.5 across a leaf's side, one leaf
    in eight transparent, one in sixteen opaque."""
    leaf_index = np.asarray(leaf_index, np.int64)
    rng = np.random.default_rng(seed)
    _, depths = oref.leaf_geometry(np.float32(scale), leaf_index)
    side = 2.0 * np.float64(np.float32(scale)) / 2.0 ** depths
    rows = np.zeros((len(leaf_index), 4), np.float32)
    rows[:, :3] = rng.random((len(leaf_index), 3), dtype=np.float32)
    kind = rng.integers(0, 16, len(leaf_index))
    sigma = (0.5 + rng.random(len(leaf_index))) / side
    sigma = np.where(kind < 2, 0.0, np.where(kind == 2, 400.0 / side, sigma))
    rows[:, 3] = sigma.astype(np.float32)
    return rows


def hand_rays():
    """``two_level_tree()`` with the densities of the K15 hand case: leaf 0 is [-1, 0]^3 (sigma 2),
    leaf 1 [0, 0.5]^3 (sigma 3), leaf 2 [0.5, 1]^3 (opaque).  One ray of each kind the kernel has a
    path for.  -> rows (3,4), starts, dirs (N,3), near, far (N,), names."""
    rows = np.float32([[0.25, 0.5, 0.75, 2.0], [1.0, 0.5, 0.0, 3.0], [0.5, 0.25, 1.0, 1e30]])
    nan = np.nan
    rays = [
        ("+x through leaf 0, zero components inside their slabs", [-2, -.5, -.5], [2, 0, 0], 0, 2),
        ("near cuts the leaf", [-2, -.5, -.5], [2, 0, 0], .75, 2),
        ("far inside the leaf", [-2, -.5, -.5], [2, 0, 0], 0, .875),
        ("far before the first leaf", [-2, -.5, -.5], [2, 0, 0], 0, .375),
        ("a start inside the cube", [-.5, -.5, -.5], [1, 1, 1], 0, 4),
        ("the diagonal through all three leaves", [-2, -2, -2], [1, 1, 1], 0, 8),
        ("a zero component outside its slab", [-2, 1.5, 0], [1, 0, 0], 0, 4),
        ("misses the cube, valid near and far", [-3, .25, .25], [1, 1.5, .125], .5, 4),
        ("a NaN direction", [-2, -.5, -.5], [nan, 1, 0], 0, 1),
        ("near beyond far", [-2, -.5, -.5], [2, 0, 0], 2, 1),
        ("through two empty octants", [.25, -.5, -.25], [0, 1, 0], 0, 2),
        ("-x through the opaque leaf", [3, .75, .8125], [-1, 0, 0], 0, 4),
        ("near and far inside one leaf", [-2, -.5, -.5], [2, 0, 0], .625, .75),
    ]
    names = [r[0] for r in rays]
    starts = np.float32([r[1] for r in rays])
    dirs = np.float32([r[2] for r in rays])
    near = np.float32([r[3] for r in rays])
    far = np.float32([r[4] for r in rays])
    return rows, starts, dirs, near, far, names


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> dict: scale, node_index, leaf_index, rows (L,4) f32, center (3,) f32, starts (WORLD: the
    centre added), directions (N,3) f32, near, far (N,) f32."""
    f32 = np.float32
    center = np.zeros(3, f32)
    if name == "hand":
        scale, nodes, leaves = two_level_tree()
        rows, starts, dirs, near, far, _ = hand_rays()
    elif name == "root":
        # depth 1: the root is the one leaf
        scale, nodes, leaves = f32(1.0), np.zeros(0, np.int64), np.zeros(1, np.int64)
        rows = f32([[0.5, 0.5, 0.5, 1.5]])
        starts, dirs = camera_rays(np.random.default_rng(7), 129, scale)
        near, far = np.zeros(129, f32), np.full(129, 4, f32)
        far[::5] = f32(2.0)                              # some end inside the leaf
        near[1::7] = f32(1.25)
    elif name in ("shell", "planes"):
        import os
        here = os.path.dirname(os.path.abspath(__file__))
        with np.load(os.path.join(here, "golden", "octree.npz")) as g:
            scale, nodes, leaves = f32(g[name + "/scale"]), g[name + "/node_index"], \
                g[name + "/leaf_index"]
        rows = leaf_rows(scale, leaves, 26)
        starts, dirs = golden_rays(name)
        starts, dirs = starts[:129].copy(), dirs[:129].copy()
        near, far = np.zeros(129, f32), np.full(129, 8, f32)
        far[::4] = f32(1.5)
        near[2::9] = f32(1.0)
        if name == "planes":
            # the cube somewhere else: the kernel subtracts the centre, the restatement gets the
            # same f32 difference
            center = f32([0.375, -1.25, 2.0])
    elif name == "mixed":
        scale, nodes, leaves = mixed_tree()
        rows = leaf_rows(scale, leaves, 27)
        starts, dirs = lattice_rays(scale, 5, 129, 26)
        near, far = np.zeros(129, f32), np.full(129, 16, f32)
        far[::3] = f32(2.5)
        near[1::4] = f32(0.75)
    else:
        raise KeyError(name)
    depth = int(oref.leaf_geometry(f32(scale), np.asarray(leaves, np.int64))[1].max()) + 1
    world = (np.asarray(starts, f32) + center[None, :]).astype(f32)
    return dict(name=name, scale=float(scale), depth=depth, node_index=np.asarray(nodes, np.int64),
                leaf_index=np.asarray(leaves, np.int64), rows=rows, center=center, starts=world,
                directions=np.asarray(dirs, f32), near=near, far=far)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 restatement of a scene, made once: -> (walk result, cdf dict)."""
    s = scene(name)
    local = (s["starts"] - s["center"][None, :]).astype(np.float32)      # the kernel's subtraction
    w = wref.walk(s["scale"], s["node_index"], s["leaf_index"], local, s["directions"])
    c = fref.cdf(w, s["scale"], local, s["directions"], s["near"], s["far"], s["rows"][:, 3])
    return w, c


def targets(rows, n_focus, seed, ends=True):
    """(rows, n_focus) f32 ascending targets in [0, 1); with ``ends`` every third row begins with
    exactly 0 and every fourth ends with exactly 1."""
    u = np.sort(np.random.default_rng(seed).random((rows, n_focus), dtype=np.float32), axis=1)
    if ends:
        u[::3, 0] = 0.0
        u[::4, -1] = 1.0
    return u


def uniform_samples(near, far, n_uniform):
    """K2a's rows without noise, numpy f32: near + linspace * (far - near); ascending, as K26 takes
    them (a row runs backwards where near lies beyond far: sorted, a no-op everywhere else)."""
    unit = np.linspace(0, 1, n_uniform, dtype=np.float32) if n_uniform > 1 else np.zeros(1, np.float32)
    near = np.asarray(near, np.float32)[:, None]
    far = np.asarray(far, np.float32)[:, None]
    with np.errstate(invalid="ignore"):
        return np.sort((near + unit[None, :] * (far - near)).astype(np.float32), axis=1)
