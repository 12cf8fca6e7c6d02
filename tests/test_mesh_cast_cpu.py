"""K36 without a GPU: the numpy restatement of the ray cast (tests/mesh_cast_reference.py) is held

* to itself: the walk through the tree gives, bit for bit, what testing every triangle gives, for
  every ``leaf_size`` and any ``order`` -- the claim that makes the tree exact;
* to ``raycast64`` of tests/mesh_raster_reference.py, the float64 caster that shares no code with it:
  the same winner on every pixel ``undecided()`` does not set aside, and ``t`` within a budget
  counted from the roundings of the chain;
* to closed forms.

The GPU tests hold the kernels to the restatement bit for bit."""

import numpy as np
import pytest

from tests import mesh_cast_reference as C
from tests import mesh_raster_reference as ref

F32 = np.float32
U = 2.0 ** -24


def _same(a, b):
    return all(np.array_equal(x.view(np.uint32) if x.dtype == F32 else x,
                              y.view(np.uint32) if y.dtype == F32 else y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------- the rays
def _axis_rays(seed, count):
    """Rays parallel to one axis (two direction components are exactly 0, either sign)."""
    rng = np.random.default_rng(seed)
    starts = rng.uniform(-1.5, 1.5, (count, 3)).astype(F32)
    directions = np.zeros((count, 3), dtype=F32)
    axis = rng.integers(0, 3, count)
    directions[np.arange(count), axis] = rng.choice([-1.0, 1.0, 0.5, -2.0], count)
    starts[np.arange(count), axis] = np.where(directions[np.arange(count), axis] > 0, -3.0, 3.0)
    return starts, directions


def _plane_rays(seed, count, bvh):
    """Rays whose origin lies exactly on a plane of a triangle's or a node's box, a third of them
    also parallel to that plane."""
    rng = np.random.default_rng(seed)
    planes = np.concatenate([bvh["boxes"], bvh["nodes"]])
    planes = planes[np.isfinite(planes).all(1)]
    starts, directions = C.random_rays(seed + 1, count)
    rows = rng.integers(0, len(planes), count)
    column = rng.integers(0, 6, count)
    axis = column % 3
    starts[np.arange(count), axis] = planes[rows, column]
    flat = np.arange(count) % 3 == 0
    directions[flat, axis[flat]] = 0.0
    # (aim the flat ones along the box, so that some of them graze it)
    return starts, directions


def _rays(seed, bvh):
    parts = [C.random_rays(seed, 120), _axis_rays(seed + 1, 60), _plane_rays(seed + 2, 90, bvh)]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


_SCENES = {}


def _scene(count):
    if count not in _SCENES:
        vertices, triangles, _, _ = ref.scene(700 + count, count)
        _SCENES[count] = (vertices, triangles)
    return _SCENES[count]


# ------------------------------------------------------------------------------- tree == brute
@pytest.mark.parametrize("leaf_size", [1, 4, 8])
@pytest.mark.parametrize("count", [1, 3, 4, 5, 300])
def test_the_tree_gives_what_testing_every_triangle_gives(count, leaf_size):
    vertices, triangles = _scene(count)
    rng = np.random.default_rng(count)
    morton = C.build(vertices, triangles, leaf_size)
    starts, directions = _rays(10 * count + leaf_size, morton)
    orders = dict(morton=None, random=rng.permutation(count).astype(np.int32),
                  reversed=np.arange(count, dtype=np.int32)[::-1].copy())
    hit_some = 0
    for farthest in (False, True):
        for t_min in (0.0, 1.5):
            want = C.brute(vertices, triangles, morton["pad"], starts, directions, t_min, farthest)
            hit_some += int((want[0] >= 0).sum())
            for name, order in orders.items():
                bvh = C.build(vertices, triangles, leaf_size, order=order)
                got = C.cast(bvh, vertices, triangles, starts, directions, t_min, farthest)
                assert _same(got, want), (name, farthest, t_min)
    assert hit_some > (0 if count < 300 else 200)


def test_the_walk_visits_every_node_at_most_once_and_culls():
    vertices, triangles = _scene(300)
    bvh = C.build(vertices, triangles, 4)
    starts, directions = C.random_rays(5, 200)
    out = C.cast(bvh, vertices, triangles, starts, directions, counts=True)
    visits, tests = out[4], out[5]
    assert visits.max() <= len(bvh["nodes"]) and visits.min() >= 1
    assert tests.max() <= 300 and tests.mean() < 0.5 * 300        # it culls
    far = np.tile(np.array([[50.0, 50.0, 50.0]], F32), (4, 1))    # rays that miss the root
    away = np.tile(np.array([[1.0, 0.5, 0.25]], F32), (4, 1))
    out = C.cast(bvh, vertices, triangles, far, away, counts=True)
    assert (out[0] == -1).all() and (out[4] == 1).all() and (out[5] == 0).all()


def test_a_parent_box_contains_its_children_and_the_slab_interval_is_monotone():
    vertices, triangles = _scene(300)
    bvh = C.build(vertices, triangles, 4)
    nodes, levels = bvh["nodes"], bvh["levels"]
    assert levels == 8 and len(nodes) == 255 and C.levels_of(300, 1) == 10 and C.levels_of(1, 4) == 1
    assert C.levels_of(4, 4) == 1 and C.levels_of(5, 4) == 2
    starts, directions = _rays(77, bvh)
    for parent in range((1 << (levels - 1)) - 1):
        ptn, ptf, _ = C.slab(nodes[parent], starts, directions)
        for child in (2 * parent + 1, 2 * parent + 2):
            if not nodes[child, 0] <= nodes[child, 3]:
                continue
            assert (nodes[parent, :3] <= nodes[child, :3]).all()
            assert (nodes[parent, 3:] >= nodes[child, 3:]).all()
            ctn, ctf, ok = C.slab(nodes[child], starts, directions)
            with np.errstate(all="ignore"):
                assert (~ok | ((ptn <= ctn) & (ctf <= ptf))).all()
    # a leaf is the hull of its triangles' boxes, leaves past the last triangle are empty
    first = (1 << (levels - 1)) - 1
    for leaf in range(1 << (levels - 1)):
        members = bvh["order"][4 * leaf:4 * leaf + 4]
        if len(members) == 0:
            assert nodes[first + leaf, 0] == np.inf and nodes[first + leaf, 3] == -np.inf
        else:
            assert np.array_equal(nodes[first + leaf, :3], bvh["boxes"][members, :3].min(0))
            assert np.array_equal(nodes[first + leaf, 3:], bvh["boxes"][members, 3:].max(0))


def test_the_keys_are_morton_codes_of_the_box_centres():
    vertices = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1023, 1023, 1023], [1024, 1024, 1024],
                         [1022, 1024, 1023], [np.nan, 0, 0]], dtype=F32)
    triangles = np.array([[0, 0, 0], [3, 3, 3], [4, 4, 4], [1, 1, 1], [2, 2, 2], [0, 1, 6]], np.int32)
    boxes, keys = C.boxes_keys(vertices, triangles, 0.0, np.zeros(3, F32), 1.0)
    assert keys.tolist() == [0, (1 << 30) - 1, (1 << 30) - 1, 1, 2, C.EMPTY_KEY]
    assert boxes[5].tolist() == [np.inf] * 3 + [-np.inf] * 3
    assert C.order_of(keys).tolist() == [0, 3, 4, 1, 2, 5]
    boxes, _ = C.boxes_keys(vertices, triangles[:1], 0.25, np.zeros(3, F32), 1.0)
    assert boxes[0].tolist() == [-0.25] * 3 + [0.25] * 3
    assert C.default_pad(vertices) == F32(2.0 ** -16) * F32(1024.0)
    lo, scale = C.grid_of(vertices)
    assert lo.tolist() == [0, 0, 0] and scale == F32(1.0)


# ------------------------------------------------------------------------------- float64
def _budget_t(tri, o, d):
    """The bound on |f32 t - float64 t| for rays (N,3) and their triangles (N,3,3), both float32
    values taken as exact, and the float64 t.

    Counting roundings, u = 2^-24, every quantity below the float64 one and |.| sums taken over
    absolute values:  e1, e2, s: one subtraction each, u |.| per component.
      p = cross(d, e2): a rounded input, two products, one subtraction: |err p_i| <= 3 u P_i,
          P_i = |d_j| |e2_k| + |d_k| |e2_j|;
      det = dot(p, e1): per term the error of p, a rounded e1 and the product, then two adds of
          partial sums: |err det| <= 7 u D, D = sum_i P_i |e1_i|;
      q = cross(s, e1): two rounded inputs: |err q_i| <= 4 u Q_i, Q_i = |s_j| |e1_k| + |s_k| |e1_j|;
      n = dot(q, e2): |err n| <= 8 u N, N = sum_i Q_i |e2_i|;
      k = 1 / det: one division; t = n k: one product:
          |err t| <= u (|t| (2 + 7 D / |det|) + 8 N / |det|).
    Doubled for the second-order terms."""
    tri, o, d = tri.astype(np.float64), o.astype(np.float64), d.astype(np.float64)
    a = tri[:, 0]
    e1, e2, s = tri[:, 1] - a, tri[:, 2] - a, o - a

    def abs_cross(x, y):
        x, y = np.abs(x), np.abs(y)
        return np.stack([x[:, 1] * y[:, 2] + x[:, 2] * y[:, 1], x[:, 2] * y[:, 0] + x[:, 0] * y[:, 2],
                         x[:, 0] * y[:, 1] + x[:, 1] * y[:, 0]], -1)

    det = (np.cross(d, e2) * e1).sum(1)
    t = (np.cross(s, e1) * e2).sum(1) / det
    big_d = (abs_cross(d, e2) * np.abs(e1)).sum(1)
    big_n = (abs_cross(s, e1) * np.abs(e2)).sum(1)
    bound = 2 * U * (np.abs(t) * (2 + 7 * big_d / np.abs(det)) + 8 * big_n / np.abs(det))
    return bound, t


@pytest.mark.parametrize("seed,count", [(11, 40), (12, 150)])
def test_the_f32_cast_agrees_with_the_float64_caster(seed, count):
    """Conditions asserted: at most 8 % of the pixels undecided, at least 45 % covered.  On every
    decided pixel the f32 winner is the float64 winner; the padded-box clause rejects none of the
    f32 triangle hits; ``t`` lies within ``_budget_t`` of float64 Moeller-Trumbore on the same
    float32 rays.  Worst use of the budget observed: 0.136 (seed 11), 0.125 (seed 12); worst
    relative error of t: 3.3e-7 and 2.4e-6."""
    width, height = 24, 20
    vertices, triangles, _, _ = ref.scene(seed, count)
    cam = ref.camera(width, height)
    winner, nearest, second = ref.raycast64(vertices, triangles, cam.intrinsics, cam.extrinsics,
                                            width, height)
    aside = ref.undecided(vertices, triangles, cam.intrinsics, cam.extrinsics, width, height,
                          nearest, second)
    print("\nscene(%d, %d): %.1f %% undecided, %.1f %% covered"
          % (seed, count, 100 * aside.mean(), 100 * (winner >= 0).mean()))
    assert aside.mean() <= 0.08 and (winner >= 0).mean() >= 0.45
    starts, directions = C.camera_rays(cam)
    bvh = C.build(vertices, triangles, 4)
    got = C.cast(bvh, vertices, triangles, starts, directions)
    assert _same(got, C.brute(vertices, triangles, bvh["pad"], starts, directions))
    assert np.array_equal(got[0][~aside], winner[~aside])

    # the padded-box clause rejects no f32 triangle hit: every (ray, triangle) pair
    tri = C.corners(vertices, triangles)
    pairs = 0
    for f in range(count):
        boxed, _, _, _ = C.hits(tri[f], bvh["boxes"][f], starts, directions, 0.0, True)
        plain, _, _, _ = C.hits(tri[f], bvh["boxes"][f], starts, directions, 0.0, False)
        assert np.array_equal(boxed, plain)
        pairs += int(plain.sum())
    assert pairs > (winner >= 0).sum()

    rows = np.flatnonzero((got[0] >= 0) & ~aside)
    budget, t64 = _budget_t(tri[got[0][rows]], starts[rows], directions[rows])
    error = np.abs(got[1][rows].astype(np.float64) - t64)
    print("t against float64: worst use of the budget %.3f, worst relative error %.3g, over %d rays"
          % ((error / budget).max(), (error / np.abs(t64)).max(), len(rows)))
    assert (error <= budget).all()
    # ... and against the caster's own depth, whose rays are not rounded to float32: the rounding of
    # the six ray components moves t by a few u times the chain's condition, the budget again
    assert (np.abs(got[1][rows] - nearest[rows]) <= 2 * budget + 8 * U * np.abs(t64)).all()


# ------------------------------------------------------------------------------- closed forms
def _cast_one(vertices, triangles, start, direction, **kwargs):
    vertices, triangles = np.asarray(vertices, F32), np.asarray(triangles, np.int32)
    bvh = C.build(vertices, triangles, kwargs.pop("leaf_size", 4))
    start, direction = np.asarray([start], F32), np.asarray([direction], F32)
    got = C.cast(bvh, vertices, triangles, start, direction, **kwargs)
    assert _same(got, C.brute(vertices, triangles, bvh["pad"], start, direction, **kwargs))
    return int(got[0][0]), float(got[1][0]), float(got[2][0]), float(got[3][0])


FAN = (np.array([[0, 0, 1], [1, 0, 1], [0, 1, 1], [-1, 0, 1], [0, -1, 1]], F32),
       np.array([[0, 1, 2], [0, 3, 4]], np.int32))


def test_a_ray_through_a_shared_vertex_goes_to_the_lower_id():
    vertices, triangles = FAN
    for leaf_size in (1, 4):
        assert _cast_one(vertices, triangles, (0, 0, 0), (0, 0, 1), leaf_size=leaf_size) \
            == (0, 1.0, 0.0, 0.0)
        assert _cast_one(vertices, triangles[::-1], (0, 0, 0), (0, 0, 1), leaf_size=leaf_size) \
            == (0, 1.0, 0.0, 0.0)
        assert _cast_one(vertices, triangles, (0, 0, 0), (0, 0, 1), farthest=True,
                         leaf_size=leaf_size) == (0, 1.0, 0.0, 0.0)
    # a shared edge: (0.5, 0, 1) lies on the edge 0-1 of triangle 0 and of its mirror image
    mirror = np.array([[0, 1, 2], [0, 4, 1]], np.int32)
    assert _cast_one(vertices, mirror, (0.5, 0, 0), (0, 0, 2))[:2] == (0, 0.5)
    assert _cast_one(vertices, mirror[::-1], (0.5, 0, 0), (0, 0, 2))[:2] == (0, 0.5)


def test_a_ray_in_the_plane_of_a_triangle_misses_it():
    vertices, triangles = FAN
    assert _cast_one(vertices, triangles[:1], (-1, 0.25, 1), (1, 0, 0)) == (-1, 0.0, 0.0, 0.0)
    assert _cast_one(vertices, triangles[:1], (0.25, 0.25, 0), (0, 0, 1)) == (0, 1.0, 0.25, 0.25)


def test_t_min_exactly_at_a_hit_excludes_it():
    vertices = np.concatenate([FAN[0][:3], FAN[0][:3] + F32([0, 0, 2])])
    triangles = np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    ray = ((0.25, 0.25, 0), (0, 0, 1))
    assert _cast_one(vertices, triangles, *ray)[:2] == (0, 1.0)
    assert _cast_one(vertices, triangles, *ray, t_min=np.nextafter(F32(1), F32(0)))[:2] == (0, 1.0)
    assert _cast_one(vertices, triangles, *ray, t_min=1.0)[:2] == (1, 3.0)
    assert _cast_one(vertices, triangles, *ray, t_min=3.0)[:2] == (-1, 0.0)
    assert _cast_one(vertices, triangles, *ray, t_min=-5.0, farthest=True)[:2] == (1, 3.0)
    # behind the origin: t < 0 is no hit for t_min = 0, and is one for t_min < t
    assert _cast_one(vertices, triangles, (0.25, 0.25, 2), (0, 0, 1))[:2] == (1, 1.0)
    assert _cast_one(vertices, triangles, (0.25, 0.25, 2), (0, 0, 1), t_min=-2.0)[:2] == (0, -1.0)


def test_the_farthest_hit_on_a_closed_box():
    vertices, triangles = C.box_mesh(1.0)
    near = _cast_one(vertices, triangles, (-3, 0.25, 0.5), (1, 0, 0))
    far = _cast_one(vertices, triangles, (-3, 0.25, 0.5), (1, 0, 0), farthest=True)
    assert near[1] == 2.0 and near[0] in (0, 1) and far[1] == 4.0 and far[0] in (2, 3)
    # from inside, every direction sees exactly one face: nearest and farthest are the same hit
    faces = set()
    for axis in range(3):
        for sign in (-1.0, 1.0):
            direction = [0.0, 0.0, 0.0]
            direction[axis] = sign
            one = _cast_one(vertices, triangles, (0.125, 0.25, -0.375), direction)
            assert one == _cast_one(vertices, triangles, (0.125, 0.25, -0.375), direction,
                                    farthest=True)
            assert one[0] // 2 == 2 * axis + (sign > 0)
            faces.add(one[0] // 2)
    assert faces == set(range(6))


def test_a_triangle_with_a_nan_vertex_is_never_hit():
    vertices, triangles, _, _ = ref.scene(31, 40)
    starts, directions = C.random_rays(32, 300)
    clean = C.brute(vertices, triangles, C.default_pad(vertices), starts, directions)
    # a large triangle in front of everything, one vertex NaN or infinite, as triangle 0
    for bad in (np.nan, np.inf, -np.inf):
        shield = np.array([[-9, -9, bad], [9, -9, 0], [0, 9, 0]], F32)
        more = np.concatenate([shield, vertices])
        ids = np.concatenate([[[0, 1, 2]], triangles + 3]).astype(np.int32)
        for leaf_size in (1, 4):
            bvh = C.build(more, ids, leaf_size)
            assert bvh["keys"][0] == C.EMPTY_KEY and bvh["order"][-1] == 0
            for farthest in (False, True):
                got = C.cast(bvh, more, ids, starts, directions, 0.0, farthest)
                want = C.brute(vertices, triangles, bvh["pad"], starts, directions, 0.0, farthest)
                assert (got[0] != 0).all()
                assert np.array_equal(got[0], np.where(want[0] >= 0, want[0] + 1, -1))
                assert _same(got[1:], want[1:])
    assert (clean[0] >= 0).sum() > 100
    # a mesh of nothing else: every node is empty, the root is not entered
    only = C.build(np.full((3, 3), np.nan, F32), np.array([[0, 1, 2]], np.int32), 4)
    out = C.cast(only, np.full((3, 3), np.nan, F32), np.array([[0, 1, 2]], np.int32), starts,
                 directions, counts=True)
    assert (out[0] == -1).all() and (out[4] == 1).all()


def test_nan_and_infinite_rays_miss():
    vertices, triangles = _scene(300)
    bvh = C.build(vertices, triangles, 4)
    starts, directions = C.random_rays(8, 12)
    starts[0, 0], starts[1, 2], directions[2, 1], directions[3, 0] = np.nan, np.inf, np.nan, -np.inf
    directions[4] = 0.0
    for farthest in (False, True):
        for t_min in (0.0, -np.inf):
            got = C.cast(bvh, vertices, triangles, starts, directions, t_min, farthest)
            assert _same(got, C.brute(vertices, triangles, bvh["pad"], starts, directions, t_min,
                                      farthest))
            assert (got[0][:5] == -1).all() and (got[1][:5] == 0).all()


def test_out_of_range_ids_are_clamped():
    vertices, triangles = _scene(5)
    wild = triangles.copy()
    wild[1, 0], wild[3, 2] = -7, 10 ** 6
    clamped = np.clip(wild, 0, len(vertices) - 1)
    starts, directions = C.random_rays(9, 200)
    bvh = C.build(vertices, wild, 4)
    assert _same(C.cast(bvh, vertices, wild, starts, directions),
                 C.brute(vertices, clamped, bvh["pad"], starts, directions))


# ------------------------------------------------------------------------------- K36d
def test_shading_blends_with_the_barycentric_weights():
    vertices, triangles = FAN
    colors = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1], [0, 0, 0]], F32)
    hit = np.array([0, -1, 1, 7], np.int32)
    t = np.array([2.5, 0, 1.5, 9], F32)
    u = np.array([0.25, 0, 0.5, 0], F32)
    v = np.array([0.5, 0, 0.5, 0], F32)
    color, alpha, depth = C.shade(hit, t, u, v, triangles, colors=colors, background=(0.5, 0.25, 1))
    assert color.tolist() == [[0.25, 0.25, 0.5], [0.5, 0.25, 1], [0.5, 0.5, 0.5], [0.5, 0.25, 1]]
    assert alpha.tolist() == [1, 0, 1, 0] and depth.tolist() == [2.5, 0, 1.5, 0]
    flat = np.full((2, 2, 3), 51, np.uint8)
    uvs = np.full((5, 2), 0.5, F32)
    color, _, _ = C.shade(hit, t, u, v, triangles, uvs=uvs, texture=flat)
    assert color[0].tolist() == [F32(51) / F32(255)] * 3 and color[1].tolist() == [0, 0, 0]


# ------------------------------------------------------------------------------- the host side
def test_the_library_and_the_wrappers_know_k36():
    from fourier_feature_nets_amd import _lib, mesh, ops
    names = ["ffn_mesh_cast_boxes", "ffn_mesh_cast_tree", "ffn_mesh_cast", "ffn_mesh_cast_shade"]
    assert set(names) <= set(_lib.declared_symbols())
    lib = _lib.load()
    for name in names:
        assert getattr(lib, name) is not None
    assert [ops.mesh_cast_levels(n, 4) for n in (1, 4, 5, 300)] == [C.levels_of(n, 4)
                                                                    for n in (1, 4, 5, 300)]
    assert ops.MESH_CAST_EMPTY_KEY == C.EMPTY_KEY
    assert mesh.MeshBVH._fields == ("nodes", "boxes", "order", "vertices", "triangles", "levels",
                                    "leaf_size", "pad")
    assert mesh.MeshHit._fields == ("triangles", "t", "u", "v")


def test_the_host_functions_refuse_by_name_without_a_device():
    import fourier_feature_nets_amd as ffn
    vertices, triangles = FAN
    for kwargs, word in ((dict(vertices=vertices[:, :2]), "vertices"),
                         (dict(triangles=triangles[:, :2]), "triangles"),
                         (dict(leaf_size=0), "leaf_size"), (dict(leaf_size=65), "leaf_size"),
                         (dict(leaf_size=2.5), "leaf_size"), (dict(pad=-1.0), "pad"),
                         (dict(pad=np.nan), "pad")):
        call = dict(vertices=vertices, triangles=triangles)
        call.update(kwargs)
        with pytest.raises(ValueError, match="build_mesh_bvh: " + word):
            ffn.build_mesh_bvh(**call)
    rays = np.zeros((4, 3), F32)
    for fn in (ffn.cast_rays, ffn.mesh_spans, ffn.render_mesh_rays):
        with pytest.raises(ValueError, match="bvh must be a MeshBVH"):
            fn(None, rays, rays)
