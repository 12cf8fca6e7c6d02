"""What the deep-tree GPU tests (tests/test_octree_deep_gpu.py, tests/test_octree_deep_mesh_gpu.py)
rest on, checked without a GPU: the embedding keeps the shallow order; the sparse K30 reference is
the dense one wherever the dense one can go, and its checkers can fail; the lattice rays of the
depth-11 tree are exact in f32; the aimed rays stay under the left-out cap by the float64 walk
alone."""

import numpy as np
import pytest

from tests import octree_deep_cases as deep
from tests import octree_mesh_reference as mref
from tests import octree_mesh_sparse_reference as sref
from tests.octree_lattice_helpers import cell_id, mixed_tree
from tests.octree_mesh_cases import CASES, case, reference


def test_embedding_keeps_the_order_and_deep11_is_the_tree_the_tests_quote():
    _, _, shallow = mixed_tree()
    nodes, leaves, slots = deep.deep11()
    assert (len(nodes), len(leaves), int(leaves[-1])) == (187, 588, 845250991)
    assert len(slots) == len(shallow) and (np.diff(slots) > 0).all()
    levels, cells = mref.leaf_levels_cells(leaves)
    s_levels, s_cells = mref.leaf_levels_cells(shallow)
    np.testing.assert_array_equal(levels[slots], s_levels + deep.DEEP11_LEVEL)
    np.testing.assert_array_equal(cells[slots], s_cells + (np.array(deep.DEEP11_AT)[None, :]
                                                          << s_levels[:, None]))
    rest = np.setdiff1d(np.arange(len(leaves)), slots)
    assert sorted(leaves[rest].tolist()) == sorted(cell_id(*c) for c in deep.DEEP11_COARSE)
    assert sorted(np.unique(levels).tolist()) == [1, 2, 3, 4, 5, 8, 9, 10]
    # every interior node is an ancestor of a leaf, every leaf's parent is a node
    assert np.isin((leaves - 1) // 8, nodes).all() and not np.isin(leaves, nodes).any()
    with pytest.raises(AssertionError):
        deep.embed(shallow, 6, deep.DEEP11_AT, [(6,) + deep.DEEP11_AT])   # a leaf inside another


@pytest.mark.parametrize("placement", mref.PLACEMENTS)
@pytest.mark.parametrize("name", CASES)
def test_the_sparse_reference_is_the_dense_one(name, placement):
    c, dense = case(name), reference(name, placement)
    sparse = sref.extract(c.scale, c.leaves, c.leaf_data, c.sh_degree, placement=placement,
                          **c.kwargs)
    for field in dense._fields:
        want, got = getattr(dense, field), getattr(sparse, field)
        if want is None:
            assert got is None
            continue
        want, got = np.asarray(want), np.asarray(got)
        assert want.shape == got.shape, field
        if field == "vertex_budget":
            assert (got <= want).all()
        elif want.dtype.kind in "iub":
            assert want.dtype == got.dtype or want.ndim == 0, field
            np.testing.assert_array_equal(got, want, err_msg=field)
        else:
            np.testing.assert_allclose(got, want, rtol=0, atol=1e-12, err_msg=field)


@pytest.mark.parametrize("depth", deep.MESH_DEPTHS)
@pytest.mark.parametrize("place", deep.MESH_PLACES)
@pytest.mark.parametrize("name", ["levels", "lone_coarse"])
def test_a_deep_tree_has_the_shallow_mesh_moved(name, place, depth):
    """What the GPU tests expect of the device, held here on the sparse reference itself."""
    m = deep.deep_mesh(name, depth, place)
    shallow = reference(name)
    got = sref.extract(m.scale, m.leaves, m.leaf_data, m.sh_degree)
    assert got.cells == 1 << (depth - 1) and got.side == shallow.side
    np.testing.assert_array_equal(got.corners, shallow.corners + m.shift)
    np.testing.assert_array_equal(got.masks, shallow.masks)
    np.testing.assert_array_equal(got.triangles, shallow.triangles)
    for field in ("offsets", "normals", "colors", "offset_budget", "normal_budget"):
        np.testing.assert_array_equal(getattr(got, field), getattr(shallow, field))
    assert got.solid_cells == shallow.solid_cells
    # the masked tree, with its mask: the mesh of the shallow tree under the same mask
    masked = deep.deep_mesh(name, depth, place, masked=True)
    assert len(masked.leaves) == len(m.leaves) + 1
    level_one = np.searchsorted(masked.leaves, [cell_id(*deep.ZERO_LEAF), cell_id(*deep.MASKED_LEAF)])
    assert not masked.solid[level_one].any() and masked.solid.sum() == (shallow.alpha > 0.5).sum()
    flagged = sref.extract(masked.scale, masked.leaves, masked.leaf_data, masked.sh_degree,
                           solid=masked.solid)
    c = case(name)
    under = sref.extract(c.scale, c.leaves, c.leaf_data, c.sh_degree, solid=masked.solid[masked.slots])
    np.testing.assert_array_equal(flagged.corners, under.corners + masked.shift)
    np.testing.assert_array_equal(flagged.triangles, under.triangles)
    # without the mask the level-1 leaf WOULD be solid, which is why no test extracts it so
    alpha = mref.opacities(masked.leaf_data, masked.sh_degree, len(masked.leaves), got.side, 0.5,
                           None)[0]
    assert alpha[np.searchsorted(masked.leaves, cell_id(*deep.MASKED_LEAF))] > 0.5
    with pytest.raises(AssertionError, match="finest cells"):
        sref.extract(masked.scale, masked.leaves, masked.leaf_data, masked.sh_degree)


def test_the_checkers_reject_wrong_answers():
    """Each is a slip a kernel could make at depth 21 and nowhere shallower."""
    m = deep.deep_mesh("levels", 21, "ones")
    ref = sref.extract(m.scale, m.leaves, m.leaf_data, m.sh_degree)
    n1 = ref.cells + 1
    keys = np.array([(i * n1 + j) * n1 + k for i, j, k in ref.corners.tolist()], np.int64)
    assert keys.max() > 2 ** 59 and ref.corners.max() == ref.cells
    sref.check_keys(keys, ref)
    sref.check_integers(ref.corners.astype(np.int32), ref.masks, ref.triangles.astype(np.int32), ref)
    with pytest.raises(AssertionError):                  # keys truncated to int32
        sref.check_keys(keys.astype(np.int32).astype(np.int64), ref)
    with pytest.raises(AssertionError):                  # keys built with 32-bit products
        sref.check_keys((keys & 0xFFFFFFFF), ref)
    with pytest.raises(AssertionError):                  # a coordinate with its top bit dropped
        sref.check_integers(ref.corners & ~(1 << 19), ref.masks, ref.triangles, ref)
    wound = ref.triangles.copy()
    wound[:2] = wound[:2][:, [0, 2, 1]]                  # one quad wound the wrong way
    with pytest.raises(AssertionError):
        sref.check_integers(ref.corners, ref.masks, wound, ref)
    assert mref.edges_pair_up(ref.triangles) and not mref.edges_pair_up(wound)
    bit = np.arange(8)
    other = (bit & 1) << 2 | (bit & 2) | (bit >> 2)      # bit dx + 2 dy + 4 dz
    swapped = (((ref.masks[:, None].astype(np.int64) >> bit) & 1) << other).sum(1).astype(np.uint8)
    assert (swapped != ref.masks).any()
    with pytest.raises(AssertionError):
        sref.check_integers(ref.corners, swapped, ref.triangles, ref)
    # the per-vertex position budget: tight (1e-5 of a cell) round the cube's centre, and what f32
    # can give (under a quarter of a cell) at its far corner, where |c - n/2| = 2^19
    centre = deep.deep_mesh("levels", 21, "centre")
    near = sref.extract(centre.scale, centre.leaves, centre.leaf_data, centre.sh_degree)
    assert near.vertex_budget.max() < 1e-4 * near.side < ref.vertex_budget.min()
    assert ref.vertex_budget.max() < 0.25 * ref.side


@pytest.mark.parametrize("name", deep.FOCUS_CASES)
def test_no_ray_of_a_focus_scene_is_undecided(name):
    from tests import octree_focus_reference as fref
    from tests.octree_focus_helpers import MIN_MASS
    s, w, c = deep.focus_scene(name)
    assert len(c["mass"]) == 4098 and not fref.undecided(c, MIN_MASS).any()
    with_mass = c["mass"] >= MIN_MASS
    assert with_mass.sum() >= 200 and (~with_mass).sum() >= 200
    assert c["count"].max() >= (12 if name in deep.AIMED_CASES else 3)


@pytest.mark.parametrize("name", deep.LATTICE_CASES)
def test_the_lattice_volume_cases_end_between_empty_and_saturated(name):
    from tests import octree_volume_reference as vref
    c = deep.walk_case(name)
    for t_min in deep.t_mins(name):
        v = vref.composite(c["w"], c["scale"], c["starts"], c["dirs"], deep.lattice_data(name),
                           t_min, (0.25, 0.5, 0.125))
        took = v["count"] > 0
        mid = took & (v["trans"] > 0.05) & (v["trans"] < 0.95)
        assert took.sum() >= 250 and mid.sum() >= 0.5 * took.sum()


@pytest.mark.parametrize("name", deep.LATTICE_CASES)
def test_the_lattice_rays_are_exact_in_f32(name):
    c = deep.walk_case(name)
    w = c["w"]
    assert deep.f32_exact(w, c["starts"], c["dirs"])
    assert w["hit"].mean() > 0.9 and (w["leaf"] >= 0).sum() > 1000
    assert (w["hit"] & (w["margin"] == 0)).sum() > 50            # ties, as on the shallow trees
    assert np.diff(w["offsets"]).max() * 3 + 2 == c["length"]
    # not exact by accident: the same rays a third of a finest cell off the lattice are not
    off = c["starts"] + np.float32(2.0 / 1024 / 3)
    from tests import octree_walk_reference as wref
    moved = wref.walk(c["scale"], c["nodes"], c["leaves"], off, c["dirs"])
    assert not deep.f32_exact(moved, off, c["dirs"])


@pytest.mark.parametrize("name", deep.AIMED_CASES)
def test_the_aimed_rays_stay_under_the_cap_by_the_reference_alone(name):
    c = deep.walk_case(name)
    w = c["w"]
    per_ray = np.diff(w["offsets"])
    leaves = np.bincount(w["ray"][w["leaf"] >= 0], minlength=len(per_ray))
    levels = mref.leaf_levels_cells(c["leaves"])[0]
    crossed = np.zeros((len(per_ray), 11), bool)
    took = w["leaf"] >= 0
    crossed[w["ray"][took], levels[w["leaf"][took]]] = True
    first, second = deep.t_mins(name)               # the very t_min the GPU tests pass
    assert first == 0.0 and 1.4 * float(c["scale"]) < second < 1.6 * float(c["scale"])
    print("%s: %.4f left out (%.4f / %.4f with t_min 0 / %.2f); %.3f meet a leaf; at most %d "
          "regions and %d leaves a ray" % (name, deep.left_out_share(c),
                                           deep.left_out_share(c, first),
                                           deep.left_out_share(c, second), second,
                                           (leaves > 0).mean(), per_ray.max(), leaves.max()))
    for t_min in (None, first, second):
        assert deep.left_out_share(c, t_min) <= deep.LEFT_OUT_CAP
    assert (leaves > 0).mean() > 0.8 and per_ray.max() >= 40 and leaves.max() >= 12
    assert per_ray.max() < 63                       # a path of 64 holds the whole chord
    assert (crossed[:, 1:6].any(1) & crossed[:, 10]).any()       # a coarse and a finest leaf
    assert c["starts"].dtype == c["dirs"].dtype == np.float32 and len(per_ray) == 4098
    norm = np.linalg.norm(c["dirs"].astype(np.float64), axis=1)
    assert np.abs(norm - 1).max() < 1e-6
    radius = np.linalg.norm(c["starts"][:4096].astype(np.float64), axis=1) / float(c["scale"])
    assert radius.min() >= 1.5 - 1e-6 and radius.max() <= 2.5 + 1e-6
