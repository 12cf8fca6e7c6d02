"""The octree walk family at ``ffn_octree_max_depth()`` = 11 on the GPU: all the modes of the walk
on ``deep11()`` (tests/octree_deep_cases.py), a sparse tree of 588 leaves whose finest cells are
2e-3 scales wide and whose largest id is 845 250 991, next to level-1 to level-5 leaves and the
large empty regions between them.

Nothing here has a tolerance of its own.  Every mode goes through the checker of that mode's
existing test, with that test's reference module and budget function:

* on the LATTICE rays (power-of-two scale; tests/test_octree_deep_cpu.py shows that f32 computes
  every crossing exactly) leaves and t are exact on every ray, ties included, as in
  tests/test_octree_lattice_gpu.py;
* on the AIMED rays, at scale 2.0 and 1.7, under the margin rule of the K13 tests.  The share of
  rays that rule leaves out may be 6 % here (2 % on the shallow trees): depth-11 cells are 2e-3
  scales wide.  The CPU test asserts the share on these very inputs by the float64 walk alone."""

import functools

import numpy as np
import pytest
import torch

from tests import octree_deep_cases as deep
from tests import octree_walk_reference as wref

pytestmark = pytest.mark.gpu

BG = (0.25, 0.5, 0.125)
CASE_T_MINS = [(name, t) for name in deep.LATTICE_CASES for t in deep.t_mins(name)]
aimed_t_mins = deep.t_mins          # the CPU test asserts the left-out shares at these very t_min


@pytest.fixture(autouse=True)
def the_cap_of_depth_eleven(monkeypatch):
    """The checkers of the shallow tests cap the left-out share at 2 %; here it is 6 %."""
    from tests import (octree_walk_helpers, test_octree_dist_gpu, test_octree_grad_gpu,
                       test_octree_refine_gpu, test_octree_render_gpu, test_octree_sh_gpu,
                       test_octree_sh_grad_gpu, test_octree_volume_gpu)
    for module in (octree_walk_helpers, test_octree_dist_gpu, test_octree_grad_gpu,
                   test_octree_refine_gpu, test_octree_render_gpu, test_octree_sh_gpu,
                   test_octree_sh_grad_gpu, test_octree_volume_gpu):
        monkeypatch.setattr(module, "LEFT_OUT_CAP", deep.LEFT_OUT_CAP)


def device_tree(c, data=True):
    import fourier_feature_nets as ffn
    return ffn.OcTree(float(c["scale"]), c["nodes"], c["leaves"], c["data"] if data else None)


def state_of(c):
    return dict(scale=c["scale"], node_index=c["nodes"], leaf_index=c["leaves"])


def ok_rays(c):
    from tests.octree_walk_helpers import ray_budget
    w = c["w"]
    return ~w["hit"] | (w["margin"] > ray_budget(w, c["scale"], c["starts"], c["dirs"]))


def wrongs(c, t_min, leaf_only=True):
    """The wrong references a lattice checker is held against.  On the whole-cube lattice the
    half-open rule turned round moves two rays in 4098, which a span or a first hit need not
    notice: there only the dropped region is used."""
    from tests.test_octree_lattice_gpu import wrong_references
    out = wrong_references(c, t_min, leaf_only)
    return out if c["name"] == "local lattice" else out[:1]


# ---------------------------------------------------------------------------- K13: path, spans
@pytest.mark.parametrize("length", [64, 6])
@pytest.mark.parametrize("name", deep.AIMED_CASES)
def test_walk_on_aimed_rays(name, length):
    from tests.octree_walk_helpers import check_walk
    c = deep.walk_case(name)
    assert device_tree(c).depth == 11
    path = device_tree(c, False).walk(c["starts"], c["dirs"], length)
    w, ok = check_walk(name, state_of(c), c["starts"], c["dirs"], length, path.t_stops, path.leaves)
    written = np.diff(w["offsets"])
    if length == 64:
        assert (written < length - 1).all() and written.max() >= 40       # the whole chord
    else:
        assert (written > length - 1).any()                               # the cap bites
    assert ok[-2:].all()                                    # the diagonal and the axis ray count


@pytest.mark.parametrize("name", deep.AIMED_CASES)
def test_spans_on_aimed_rays(name):
    """The span assertions of ``test_walk_on_large_random_clouds``."""
    from tests.octree_walk_helpers import ray_budget
    c = deep.walk_case(name)
    w, ok = c["w"], ok_rays(c)
    tree = device_tree(c, False)
    starts, directions = c["starts"], c["dirs"]
    budget = ray_budget(w, tree.scale, starts, directions)
    for t_min, pad in [(0.0, 0.0), (0.0, 1.0), (aimed_t_mins(name)[1], 2.5)]:
        t_in, t_out, hit = tree.spans(starts, directions, t_min, pad)
        assert t_in.dtype == np.float32 and hit.dtype == np.bool_
        want_in, want_out, want_hit = wref.spans(w, tree.scale, tree.depth, directions, t_min, pad)
        near_t_min = np.zeros(len(ok), bool)
        close = (w["leaf"] >= 0) & (np.abs(w["t_out"] - t_min) <= budget[w["ray"]])
        near_t_min[w["ray"][close]] = True
        rows = ok & ~near_t_min
        assert (1.0 - rows.mean()) <= deep.LEFT_OUT_CAP
        assert np.array_equal(hit[rows], want_hit[rows])
        both = rows & want_hit
        width = np.abs(want_out - want_in) * 2.0 ** -22          # pad: one multiply, one add
        worst = max(np.abs(t_in - want_in)[both].max(), np.abs(t_out - want_out)[both].max())
        print("%s spans(t_min %.2f, pad %.1f): %d of %d rays hit, %.4f left out; worst error %.3g "
              "(smallest budget %.3g)" % (name, t_min, pad, hit.sum(), len(hit), 1 - rows.mean(),
                                          worst, budget[both].min()))
        assert (np.abs(t_in - want_in) <= budget + width)[both].all()
        assert (np.abs(t_out - want_out) <= budget + width)[both].all()
        assert (t_in[~hit] == 0).all() and (t_out[~hit] == 0).all()


@pytest.mark.parametrize("name", deep.LATTICE_CASES)
def test_lattice_paths_are_exact_on_every_ray(name):
    from tests.test_octree_lattice_gpu import bits, check_path
    c = deep.walk_case(name)
    tree = device_tree(c, False)
    path = tree.walk(c["starts"], c["dirs"], c["length"])
    gone = check_path(c, c["w"], path.t_stops, path.leaves)
    print("%s: %d rays (%d hit, %d with margin 0), longest %d regions, %d zero-length stops, all "
          "touches" % (name, len(c["starts"]), c["w"]["hit"].sum(),
                       (c["w"]["hit"] & (c["w"]["margin"] == 0)).sum(),
                       np.diff(c["w"]["offsets"]).max(), gone))
    for short in (3, 6):
        cut = tree.walk(c["starts"], c["dirs"], short)
        assert np.array_equal(bits(cut.t_stops[:, :short - 1]), bits(path.t_stops[:, :short - 1]))
        assert np.array_equal(cut.leaves[:, :short - 1], path.leaves[:, :short - 1])
        assert np.array_equal(bits(cut.t_stops[:, -1]), bits(path.t_stops[:, -1]))
        assert (cut.leaves[:, -1] == -1).all()
    for what, wrong in wrongs(c, 0.0, leaf_only=False):
        with pytest.raises(AssertionError):
            check_path(c, wrong, path.t_stops, path.leaves)


@pytest.mark.parametrize("name,t_min", CASE_T_MINS)
def test_lattice_spans_first_hit_and_render_are_exact_on_every_ray(name, t_min):
    from fourier_feature_nets_amd import ops
    from tests import octree_render_reference as rref
    from tests.test_octree_lattice_gpu import bits, check_first, check_spans
    from tests.test_octree_render_gpu import check_first_hit
    c = deep.walk_case(name)
    w = c["w"]
    tree = device_tree(c)
    got = tree.spans(c["starts"], c["dirs"], t_min, 0.0)
    early, late, only = check_spans(c, w, t_min, *got)
    hit = tree.first_hit(c["starts"], c["dirs"], t_min)
    touches = check_first(c, w, t_min, hit.leaves, hit.t, hit.faces)
    found = hit.leaves >= 0
    print("%s t_min=%.4f: %d rays hit a leaf, %d of them a touched one; %d spans begin and %d end "
          "at a touched leaf" % (name, t_min, found.sum(), touches, early, late))
    assert found.sum() > 40
    assert np.array_equal(got[2], found) and np.array_equal(bits(got[0][found]), bits(hit.t[found]))
    # the colour: the leaf's, times the shade of the reported face
    shade = ops.octree_face_shade()
    out = tree.render(c["starts"], c["dirs"], t_min, background=BG, shading="faces")
    rgb = c["data"][np.maximum(hit.leaves, 0), :3]
    want = np.where(found[:, None], rgb * shade[np.maximum(hit.faces, 0)][:, None],
                    np.float32(BG)[None, :]).astype(np.float32)
    assert np.array_equal(bits(out.color), bits(want))
    assert np.array_equal(out.alpha, found.astype(np.float32))
    assert np.array_equal(bits(out.depth), bits(hit.t))
    # the first qualifying stop of K13, bit for bit
    path = tree.walk(c["starts"], c["dirs"], c["length"])
    takes = (path.leaves[:, :-1] >= 0) & (path.t_stops[:, 1:] > np.float32(t_min))
    assert np.array_equal(takes.any(1), found)
    k = takes.argmax(1)
    rows = np.arange(len(k))
    assert np.array_equal(path.leaves[rows, k][found], hit.leaves[found])
    free = found & (hit.faces != 6)
    # ``first_hit`` returns ``max(entry t, t_min)``: an entry at -0 with t_min = +0 gives +0, while
    # the walk stores the crossing itself.  Nothing else may differ.
    stop_t = path.t_stops[rows, k][free]
    differ = bits(stop_t) != bits(hit.t[free])
    assert (bits(stop_t[differ]) == 0x80000000).all() and (bits(hit.t[free][differ]) == 0).all()
    assert t_min == 0.0 or not differ.any()
    assert (path.t_stops[rows, k][found & ~free] < np.float32(t_min)).all()
    # the rays without any tie, through the checker of the other first-hit tests
    want = rref.first_hit(w, c["scale"], c["leaves"], c["starts"], c["dirs"], t_min)
    plain = ~w["hit"] | (w["margin"] > 0) & (want["edge_gap"] > 0)
    sub = wref.walk(c["scale"], c["nodes"], c["leaves"], c["starts"][plain], c["dirs"][plain])
    check_first_hit(name + ", no tie", state_of(c), c["starts"][plain], c["dirs"][plain], t_min,
                    type(hit)(hit.leaves[plain], hit.t[plain], hit.faces[plain]), sub,
                    every_ray=True)
    for what, wrong in wrongs(c, t_min):
        with pytest.raises(AssertionError):
            check_spans(c, wrong, t_min, *got)
        with pytest.raises(AssertionError):
            check_first(c, wrong, t_min, hit.leaves, hit.t, hit.faces)


# -------------------------------------------------------------------------- K14: first hit
@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("name", deep.AIMED_CASES)
def test_first_hit_and_render_on_aimed_rays(name, which):
    from fourier_feature_nets_amd import ops
    from tests.test_octree_render_gpu import bits, check_first_hit
    c = deep.walk_case(name)
    t_min = aimed_t_mins(name)[which]
    tree = device_tree(c)
    hit = tree.first_hit(c["starts"], c["dirs"], t_min)
    check_first_hit(name, state_of(c), c["starts"], c["dirs"], t_min, hit, c["w"])
    assert (hit.leaves >= 0).sum() > 2500 and (which == 0 or (hit.faces == 6).any())
    assert len(np.unique(hit.faces[hit.faces >= 0])) >= 6
    # ``render`` shades that very hit: the leaf's colour times the shade of the reported face
    found = hit.leaves >= 0
    out = tree.render(c["starts"], c["dirs"], t_min, background=BG, shading="faces")
    rgb = c["data"][np.maximum(hit.leaves, 0), :3]
    want = np.where(found[:, None], rgb * ops.octree_face_shade()[np.maximum(hit.faces, 0)][:, None],
                    np.float32(BG)[None, :]).astype(np.float32)
    assert np.array_equal(bits(out.color), bits(want))
    assert np.array_equal(out.alpha, found.astype(np.float32))
    assert np.array_equal(bits(out.depth), bits(hit.t))


# ------------------------------------------------------------------ K15 / K18: volume, plain and SH
@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("name", deep.AIMED_CASES)
def test_volume_on_aimed_rays(name, which):
    from tests.test_octree_volume_gpu import check_volume
    c = deep.walk_case(name)
    t_min = aimed_t_mins(name)[which]
    out = device_tree(c).render_volume(c["starts"], c["dirs"], t_min, BG)
    v, _ = check_volume(name, state_of(c), c["data"], c["starts"], c["dirs"], t_min, out, c["w"])
    assert v["count"].max() >= 12                       # a dozen leaves and more in one ray


@pytest.mark.parametrize("name,t_min", CASE_T_MINS)
def test_volume_on_lattice_rays(name, t_min):
    """Every ray, ties included.  ``lattice_data``: the densities at which these rays end neither
    empty nor saturated (tests/test_octree_deep_cpu.py)."""
    import fourier_feature_nets as ffn
    from tests.test_octree_volume_gpu import check_volume
    c = deep.walk_case(name)
    data = deep.lattice_data(name)
    tree = ffn.OcTree(float(c["scale"]), c["nodes"], c["leaves"], data)
    out = tree.render_volume(c["starts"], c["dirs"], t_min, BG)
    check_volume(name, state_of(c), data, c["starts"], c["dirs"], t_min, out, c["w"],
                 every_ray=True)
    for what, wrong in wrongs(c, t_min):
        with pytest.raises(AssertionError):
            check_volume(name, state_of(c), data, c["starts"], c["dirs"], t_min, out, wrong,
                         every_ray=True)


@pytest.mark.parametrize("degree", [1, 2])
@pytest.mark.parametrize("name,t_min", CASE_T_MINS)
def test_sh_volume_and_gradient_on_lattice_rays(name, t_min, degree):
    """Every ray counts (``ok`` is all true): the crossings are exact."""
    import fourier_feature_nets as ffn
    from tests.octree_sh_helpers import sh_leaf_data
    from tests.test_octree_sh_gpu import check_sh
    from tests.test_octree_sh_grad_gpu import check
    c = deep.walk_case(name)
    data = sh_leaf_data(c["scale"], c["leaves"], degree)
    # ``sh_leaf_data`` has eight times the plain density already
    data[:, -1] *= np.float32(max(deep.LATTICE_DENSITY_GAIN[name] / 8.0, 1.0))
    every = np.ones(len(c["starts"]), bool)
    tree = ffn.OcTree(float(c["scale"]), c["nodes"], c["leaves"], data, sh_degree=degree)
    got = tree.render_volume(c["starts"], c["dirs"], t_min, BG)
    v = check_sh(name, c["scale"], data, degree, c["starts"], c["dirs"], t_min, got, c["w"], every)
    assert (v["count"] > 0).sum() >= 250
    for min_t in (0.0, 1e-3):
        _, g, _ = check(name, c["scale"], c["nodes"], c["leaves"], data, degree, c["starts"],
                        c["dirs"], c["w"], every, t_min, min_t)
        assert (g["taken"] > 0).sum() >= 3


@pytest.mark.parametrize("degree", [1, 2])
@pytest.mark.parametrize("name", deep.AIMED_CASES)
def test_sh_volume_on_aimed_rays(name, degree):
    import fourier_feature_nets as ffn
    from tests.octree_sh_helpers import sh_leaf_data
    from tests.test_octree_sh_gpu import check_sh
    c = deep.walk_case(name)
    data = sh_leaf_data(c["scale"], c["leaves"], degree)
    tree = ffn.OcTree(float(c["scale"]), c["nodes"], c["leaves"], data, sh_degree=degree)
    for t_min in aimed_t_mins(name):
        got = tree.render_volume(c["starts"], c["dirs"], t_min, BG)
        check_sh(name, c["scale"], data, degree, c["starts"], c["dirs"], t_min, got, c["w"],
                 ok_rays(c))


# ------------------------------------------------------------ K17 / K19 / K29: the backward passes
@pytest.mark.parametrize("which,min_t", [(0, 0.0), (1, 1e-3)])
@pytest.mark.parametrize("name", deep.AIMED_CASES)
def test_gradient_on_aimed_rays(name, which, min_t):
    from tests.test_octree_grad_gpu import check_gradient
    c = deep.walk_case(name)
    check_gradient(name, device_tree(c), c["data"], c["starts"], c["dirs"], c["w"],
                   aimed_t_mins(name)[which], min_t)


@pytest.mark.parametrize("name,t_min", CASE_T_MINS)
def test_gradient_on_lattice_rays(name, t_min):
    from tests.test_octree_grad_gpu import check_gradient
    c = deep.walk_case(name)
    tree = device_tree(c)
    for min_t in (0.0, 1e-3):
        check_gradient(name, tree, c["data"], c["starts"], c["dirs"], c["w"], t_min, min_t,
                       share=False, every_ray=True)
    if name == "local lattice":
        for what, wrong in wrongs(c, t_min):
            with pytest.raises(AssertionError):
                check_gradient(name, tree, c["data"], c["starts"], c["dirs"], wrong, t_min, 0.0,
                               share=False, every_ray=True)


@pytest.mark.parametrize("degree", [1, 2])
@pytest.mark.parametrize("name", deep.AIMED_CASES)
def test_sh_gradient_on_aimed_rays(name, degree):
    from tests.octree_sh_helpers import sh_leaf_data
    from tests.test_octree_sh_grad_gpu import check
    c = deep.walk_case(name)
    data = sh_leaf_data(c["scale"], c["leaves"], degree)
    for t_min, min_t in ((0.0, 0.0), (aimed_t_mins(name)[1], 1e-3)):
        check(name, c["scale"], c["nodes"], c["leaves"], data, degree, c["starts"], c["dirs"],
              c["w"], ok_rays(c), t_min, min_t)


@functools.lru_cache(maxsize=None)
def dist_case(name):
    from tests.octree_dist_helpers import Case
    c = deep.walk_case(name)
    made = Case(c["scale"], c["nodes"], c["leaves"], c["data"], c["starts"], c["dirs"],
                every_ray=name in deep.LATTICE_CASES)
    assert made.depth == 11
    return made


@pytest.mark.parametrize("name", deep.AIMED_CASES + deep.LATTICE_CASES)
def test_distortion_forward_and_backward_plain_and_sh(name, monkeypatch):
    """The K29 tests' own bodies on the deep tree: the ray distortion and its gradient with zero
    upstream, the backward with random upstream and the term (each leaf within K17's budget plus
    the term's), and SH rows with the same densities."""
    from tests import test_octree_dist_gpu as dist
    monkeypatch.setattr(dist, "case", dist_case)
    for t_min, min_t in zip(deep.t_mins(name), (0.0, 1e-3)):
        _, ref, _ = dist.check_case(name, t_min, min_t)
        # the whole-cube lattice meets the five coarse leaves and a few of the fine ones
        assert (ref["taken"] > 0).sum() > (100 if t_min == 0 and name != "cube lattice" else 4)
        dist.test_backward_with_random_upstream(name, t_min, min_t)
    for degree in (1, 2):
        dist.test_sh_rows(name, degree)


# ------------------------------------------------------------------------- K21a: leaf weights
@pytest.mark.parametrize("name", deep.AIMED_CASES)
def test_leaf_weights_on_aimed_rays(name):
    from tests.test_octree_refine_gpu import check_weights, expected_weights, sure_rays
    c = deep.walk_case(name)
    starts, dirs, w = sure_rays(c["scale"], c["nodes"], c["leaves"], c["starts"], c["dirs"])
    tree = device_tree(c)
    for t_min, min_t in ((0.0, 0.0), (aimed_t_mins(name)[1], 0.5)):
        if t_min > 0:
            # ``expected_weights`` asserts that half the leaves are seen, which holds from t = 0
            from tests import octree_refine_reference as rref
            want, budget, taken, _ = rref.leaf_max_weights(w, c["scale"], starts, dirs, c["data"],
                                                           len(c["leaves"]), t_min, min_t)
        else:
            want, budget, taken = expected_weights(name, c["scale"], c["leaves"], c["data"], starts,
                                                   dirs, w, t_min, min_t)
        check_weights(name, tree.leaf_weights(starts, dirs, t_min, min_t), want, budget, taken)
        assert taken.sum() > 100


@pytest.mark.parametrize("name,t_min", CASE_T_MINS)
def test_leaf_weights_on_lattice_rays(name, t_min):
    """Every ray, ties included: a leaf that a ray only touches has a chord of 0 and weight +0."""
    import fourier_feature_nets as ffn
    from tests import octree_refine_reference as rref
    from tests.test_octree_refine_gpu import check_weights
    c = deep.walk_case(name)
    data = deep.lattice_data(name)
    tree = ffn.OcTree(float(c["scale"]), c["nodes"], c["leaves"], data)
    for min_t in (0.0, 0.5):
        want, budget, taken, _ = rref.leaf_max_weights(c["w"], c["scale"], c["starts"], c["dirs"],
                                                       data, len(c["leaves"]), t_min, min_t)
        print("%s t_min=%.4f min_T=%.1f: %d of %d leaves taken" % (name, t_min, min_t, taken.sum(),
                                                                  len(taken)))
        check_weights(name, tree.leaf_weights(c["starts"], c["dirs"], t_min, min_t), want, budget,
                      taken)
        assert taken.sum() >= 5 and (want > 0).sum() >= 5


# ------------------------------------------------------------------------- K26: focus samples
@pytest.mark.parametrize("n_focus,n_uniform", [(64, 0), (3, 64)])
@pytest.mark.parametrize("name", deep.FOCUS_CASES)
def test_focus_samples(name, n_focus, n_uniform):
    """All 4098 rays of every walk case, aimed (both scales) and lattice, in chunks that are no
    multiple of a wave.  The focus reference takes any ray: its budgets come from the crossings'
    own, so the lattice rays need no rule of their own."""
    from tests import octree_focus_reference as fref
    from tests.octree_focus_helpers import MIN_MASS, targets, uniform_samples
    from tests.test_octree_focus_gpu import bits, run, subset
    s, _, c = deep.focus_scene(name)
    total = len(s["near"])
    worst = 0.0
    for first in range(0, total, 1025):
        index = np.arange(first, min(first + 1025, total))
        rays = len(index)
        u = targets(rays, n_focus, 1000 + first + n_focus)
        near, far = s["near"][index], s["far"][index]
        t, mass = run(s, index, u)
        assert t.shape == (rays, n_focus) and t.dtype == np.float32 and mass.shape == (rays,)
        worst = max(worst, fref.check(subset(c, index), near, far, u, MIN_MASS, t, mass, name))
        if n_uniform and first == 0:
            wide = np.full((rays, n_uniform + 3), np.float32(-7.0))
            wide[:, :n_uniform] = uniform_samples(near, far, n_uniform)
            merged, mass_merged = run(s, index, u, wide, n_uniform)
            want = np.sort(np.concatenate([wide[:, :n_uniform], t], axis=1), axis=1)
            assert (bits(merged) == bits(want)).all() and (bits(mass_merged) == bits(mass)).all()
    with_mass = (c["mass"] >= MIN_MASS).sum()
    print("%s n_focus=%d: %d rays, %d with mass, at most %d leaves a ray; worst |F(t) - u M| / "
          "budget %.3f" % (name, n_focus, total, with_mass, c["count"].max(), worst))
    assert with_mass >= 200 and total == 4098


# ------------------------------------------------------------- K24 / K28: visible votes and moments
def visible_scene():
    import fourier_feature_nets as ffn
    from tests.visible_helpers import densities
    nodes, leaves, _ = deep.deep11()
    scale = np.float32(1.7)
    cameras = deep.cell_cameras(scale, deep.VISIBLE_EYES, 0.5)
    return (scale, nodes, leaves, densities(scale, 11, len(leaves), 3), cameras,
            ffn.projection_matrices(cameras), ffn.eye_positions(cameras, (0, 0, 0)))


@pytest.mark.parametrize("tau", [0.0, 0.3])
def test_visible_votes_and_moments(tau):
    from tests import photo_reference as pref
    from tests.carve_helpers import seeded_images
    from tests.photo_helpers import rgba_images
    from tests.test_octree_photo_gpu import kernel, plain_rows
    from tests.test_octree_visible_gpu import against_reference
    scale, nodes, leaves, density, cameras, proj, eyes = visible_scene()
    assert [(c.resolution.width, c.resolution.height) for c in cameras] == [(24, 20)] * 3
    want, _ = against_reference(scale, nodes, leaves, density, seeded_images(3, 20, 24, 2, fill=0.9),
                                cameras, 128, tau)
    assert 0 < want["visible"].sum() <= want["candidate"].sum() < want["pairs"]
    assert tau == 0.0 or want["visible"].sum() < want["candidate"].sum()
    images = rgba_images(3, 20, 24, 5, 128)
    want = pref.moments(scale, nodes, leaves, density, images, proj, eyes, 128, tau)
    print("moments, tau %.1f: %d leaves x 3 cameras, %d undecided, %d candidates, %d visible"
          % (tau, len(leaves), int(want["undecided"].sum()), int(want["candidate"].sum()),
             int(want["visible"].sum())))
    assert want["undecided"].sum() <= 0.01 * want["undecided"].size
    got = kernel(scale, nodes, leaves, plain_rows(density), images, proj, eyes, 128, tau)
    got = got.cpu().numpy().astype(np.int64)
    sure = ~want["undecided"].any(1)
    assert np.array_equal(got[sure], want["moments"][sure])
    assert (got[:, 3] > 1).sum() > 50


# -------------------------------------------------- the tree as it is: neighbours, TV, occupancy
def test_neighbors_and_total_variation():
    import fourier_feature_nets as ffn
    from fourier_feature_nets_amd import ops
    from tests import octree_tv_reference as tref
    nodes, leaves, _ = deep.deep11()
    nb, edge_list = tref.tree_edges(nodes, leaves)
    tree = ffn.OcTree(2.0, nodes, leaves)
    got = tree.neighbors()
    assert got.dtype == np.int64 and got.shape == (len(leaves), 6)
    assert np.array_equal(got, nb)
    plan = tree._tv_plan()
    assert plan.num_edges == len(edge_list) and plan.num_leaves == len(leaves)
    assert np.array_equal(torch.stack([plan.edge_i, plan.edge_j], 1).cpu().numpy(), edge_list)
    level = tref.levels(leaves)
    assert (level[edge_list[:, 0]] != level[edge_list[:, 1]]).any()
    for stride, eps in ((4, 1e-3), (28, 1e-1)):
        rows = np.random.default_rng(3).normal(size=(len(leaves), stride)).astype(np.float32)
        lam = np.float32([1.0, 0.0, 0.5, 2.0]) if stride == 4 else \
            ops.octree_tv_weights((1.0, 0.0, 2.0), stride, 2)
        want = tref.total_variation(rows, edge_list, lam, eps)
        assert plan.longest == int(want["incidences"].max())
        value, grad = ops.octree_tv(torch.from_numpy(rows).cuda(), plan, lam, eps)
        value, grad = float(value.item()), grad.cpu().numpy()
        err = np.abs(grad.astype(np.float64) - want["grad"])
        print("deep11 stride %d eps %g: %d edges, longest list %d; R off by %.3g of a budget of "
              "%.3g; worst row entry at %.3g of its budget"
              % (stride, eps, len(edge_list), plan.longest, abs(value - want["value"]),
                 want["value_budget"], float((err / np.maximum(want["budget"], 1e-300)).max())))
        assert abs(value - want["value"]) <= want["value_budget"]
        assert (err <= want["budget"]).all()


def test_occupancy_grid_from_the_tree():
    from fourier_feature_nets_amd import ops
    from tests import occupancy_octree_reference as kref
    nodes, leaves, _ = deep.deep11()
    centre, half = deep.cell_box(2.0, deep.DEEP11_AT, deep.DEEP11_LEVEL)
    lo = tuple(float(np.float32(v - 1.25 * half)) for v in centre)
    places = {"the cube": (2.0, (0.0, 0.0, 0.0), (-2.0, -2.0, -2.0), (4.0, 4.0, 4.0)),
              "round the cell": (2.0, (0.0, 0.0, 0.0), lo, (float(np.float32(2.5 * half)),) * 3)}
    ids = torch.from_numpy(leaves).cuda()
    for what, (scale, center, box_min, box_size) in places.items():
        want = kref.Rule().words(leaves, scale, center, box_min, box_size, 32, None, None, 0)
        got = ops.occupancy_from_octree(ids, scale, center, box_min, box_size, 32)
        got = got.cpu().numpy().view(np.uint32)
        set_bits = int(np.unpackbits(want.view(np.uint8)).sum())
        print("occupancy %s: %d of %d cells set" % (what, set_bits, 32 ** 3))
        assert 0 < set_bits < 32 ** 3
        assert np.array_equal(got, want)


# ------------------------------------------- the grid builders at the top of the depth-11 codes
def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda").contiguous()


def test_cell_centers_and_density_select_at_the_last_codes():
    from fourier_feature_nets_amd import ops
    from fourier_feature_nets_amd._lib import FfnError
    from tests import octree_density_reference as dref
    from tests import octree_reference as oref
    from tests.test_octree_density_gpu import bits
    first, count, depth = deep.TOP_FIRST, deep.TOP_COUNT, 11
    assert first + count == 8 ** 10 == 2 ** 30 and count % 64 != 0
    scale = float(np.float32(deep.TOP_SCALE))
    got = ops.octree_cell_centers(first, count, deep.TOP_CENTER, scale, depth, "cuda").cpu().numpy()
    # the f32 chain of tests/octree_reference.py, and the centre added in f32
    ids = np.arange(first, first + count, dtype=np.int64) + dref.first_id(depth - 1)
    chain, depths = oref.leaf_geometry(np.float32(scale), ids)
    assert chain.dtype == np.float32 and (depths == depth - 1).all()
    assert np.array_equal(bits(got), bits(chain + np.float32(deep.TOP_CENTER)[None, :]))
    assert np.array_equal(bits(got), bits(dref.cell_centers(first, count, deep.TOP_CENTER, scale,
                                                            depth)))
    # K16b on seeded logits that keep about half the cells
    logits = np.random.default_rng(100 + count).normal(size=(count, 4)).astype(np.float32) * 3
    side, tau = dref.side_of(scale, depth), dref.tau_of(0.01)
    logits[:, 3] += np.float32(np.log(np.expm1(float(tau) / float(side))))     # softplus^-1(tau/side)
    baked = ops.octree_bake(dev(logits)).cpu().numpy()
    want_codes, want_data = dref.select(baked, first, tau, side)
    codes, data = ops.octree_density_select(dev(logits), first, float(tau), float(side), depth)
    print("density select at the last codes: %d of %d kept, largest code %d"
          % (len(want_codes), count, want_codes.max()))
    assert 0.3 * count < len(want_codes) < 0.7 * count
    assert codes.dtype == torch.int32 and np.array_equal(codes.cpu().numpy(), want_codes)
    assert np.array_equal(bits(data.cpu().numpy()), bits(want_data))
    # everything kept: the largest code is 2^30 - 1, as an int32
    logits[:, 3] = 30.0
    codes, _ = ops.octree_density_select(dev(logits), first, float(tau), float(side), depth)
    assert codes.dtype == torch.int32
    assert np.array_equal(codes.cpu().numpy(), np.arange(first, first + count))
    assert int(codes[-1]) == 2 ** 30 - 1
    # one past the end is refused by the argument checks, which run before any launch
    with pytest.raises(ValueError, match="first_code"):
        ops.octree_cell_centers(first + 1, count, deep.TOP_CENTER, scale, depth, "cuda")
    with pytest.raises(FfnError, match="codes inside"):
        ops.octree_density_select(dev(logits), first + 1, float(tau), float(side), depth)


def test_carve_select_and_carve_box_at_the_last_codes():
    from fourier_feature_nets_amd import ops
    from tests.test_octree_carve_box_gpu import same_as_restatement as same_box
    from tests.test_octree_carve_gpu import same_as_restatement as same_point
    first, count, depth = deep.TOP_FIRST, deep.TOP_COUNT, 11
    images, mask, proj = deep.top_scene()
    for max_misses, min_views in ((1, 3), (1, 2)):
        codes, data, visited = same_point(images, mask, proj, first, count, deep.TOP_CENTER,
                                          deep.TOP_SCALE, depth, 128, max_misses, min_views)
        print("carve_select at the last codes (%d, %d): %d of %d kept, largest %d"
              % (max_misses, min_views, len(codes), count, codes.max()))
        assert codes.dtype == np.int32 and 0 < len(codes) < count
        assert first <= codes.min() and (np.diff(codes) > 0).all()
        assert visited.max() == 3                      # the + corner projects inside all images
        assert codes.max() == 2 ** 30 - 1              # the last cell of the grid is kept
    with pytest.raises(ValueError, match="leave the"):
        ops.octree_carve_select(dev(images), dev(mask), dev(proj), first + 1, count,
                                deep.TOP_CENTER, deep.TOP_SCALE, depth, 128, 1, 2, 1.25)
    # K27 on the same cells: mostly background, so that rectangles of a few pixels can be empty
    images, _, proj = deep.top_scene(fill=0.06)
    mask = (images[..., 3] >= 128).astype(np.uint8)
    tested = np.arange(first, first + count)
    for max_misses, min_views in ((0, 3), (1, 1)):
        kept, rows = same_box(images, mask, proj, tested, depth - 1, deep.TOP_CENTER,
                              deep.TOP_SCALE, depth, max_misses, min_views)
        print("carve_box at the last codes (%d, %d): %d of %d kept, largest %d"
              % (max_misses, min_views, len(kept), count, kept.max()))
        # ``same_box`` holds the device codes to int32 and to ``tested[keep]``, that is first + i
        assert 0 < len(kept) < count and kept.min() >= first
        assert kept.max() == 2 ** 30 - 1               # the last cell of the grid is kept
    # the parents of those cells, expanded: the children's codes pass 2^27 * 8
    parents = np.arange(first >> 3, (first + count) >> 3)
    same_box(images, mask, proj, parents, depth - 1, deep.TOP_CENTER, deep.TOP_SCALE, depth, 1, 1,
             expand=True)
