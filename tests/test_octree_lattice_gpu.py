"""All five modes of the octree walk (K13 path and spans, K14 first hit and render, K15 volume,
K17 gradient) on rays with EXACT answers: the lattice rays of tests/octree_lattice_helpers.py,
where two or three planes tie at one t all the time.  No ray is left out and no t carries a
tolerance: every crossing is a small dyadic number, the same in f32 and in the float64
restatement (tests/octree_walk_reference.py).  No reference file is read.

What a tie leaves open, and what is therefore accepted:

* a ZERO-LENGTH stop.  Leaving a region through an edge or a corner the walk crosses one plane
  at a time, so it may own for no length a region the ray only touches (the float64 slab test
  of the region's CLOSED box has ``t_out == t_in``).  Such stops are deleted before the path is
  compared, and each of them must be such a touch; a touched leaf may begin a span, end it, or be
  a first hit at its touch point, and carries weight 0 in the volume and the gradient;
* the entry FACE of a ray that enters its leaf through an edge or a corner: any tied axis.

The volume and gradient comparisons keep the budgets of their own restatements
(tests/octree_volume_reference.py, tests/octree_grad_reference.py); on these rays the crossing
terms of those budgets are slack and the compositing terms are what is tested."""

import functools

import numpy as np
import pytest
import torch

from tests import octree_reference as oref
from tests import octree_render_reference as rref
from tests import octree_volume_reference as vref
from tests import octree_walk_reference as wref
from tests.octree_lattice_helpers import closed_touch, lattice_rays, mixed_tree
from tests.octree_volume_helpers import hand_case, random_leaf_data

pytestmark = pytest.mark.gpu

BG = (0.25, 0.5, 0.125)
T_MINS = [0.0, 1.25]                 # 1.25: a lattice value that lies inside leaves on many rays
CASES = ["hand case", "mixed", "root only"]


def bits(x):
    if torch.is_tensor(x):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def exact(got, want):
    """f32 ``got`` equals float64 ``want`` BIT FOR BIT wherever ``want`` is not zero.  Where it is
    zero ``got`` must be a zero, of either sign: a crossing ``(plane - o) / d`` with ``plane == o``
    is -0 for ``d < 0`` and +0 for ``d > 0``, and when two such axes tie which of them gives the
    t is the walk's order of axes on one side and that of ``min`` / ``max`` on the other -- no
    contract.  (Not finite: the same value.)"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float64)
    zero = want == 0
    with np.errstate(over="ignore", invalid="ignore"):
        same = bits(got) == bits(want.astype(np.float32))
    return got.shape == want.shape and bool((same[~zero]).all()) and bool((got[zero] == 0).all()) \
        and np.array_equal(got.astype(np.float64)[~zero], want[~zero])


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict: the tree's arrays, depth, leaf data (L,4), rays and their restatement.  Ray counts:
    64 k + 1, 64 k and 64 k + 1."""
    if name == "hand case":
        # two_level_tree() with the hand case's data (its opaque leaf made finite) and its five
        # hand-worked rays in front of the lattice rays
        scale, nodes, leaves, data, hand_s, hand_d = hand_case()
        data = data.copy()
        data[2, 3] = 1.5
        starts, dirs = lattice_rays(scale, 3, 2044, 21)
        starts, dirs = np.concatenate([hand_s, starts]), np.concatenate([hand_d, dirs])
        depth = 3
    elif name == "mixed":
        scale, nodes, leaves = mixed_tree()
        depth = 5
        data = random_leaf_data(scale, leaves)
        starts, dirs = lattice_rays(scale, depth, 4096, 22)
    else:
        scale, nodes, leaves = np.float32(2.0), np.zeros(0, np.int64), np.array([0], np.int64)
        depth = 1
        data = np.float32([[0.5, 0.25, 1.0, 0.2]])
        starts, dirs = lattice_rays(scale, depth, 1025, 23)
    w = wref.walk(scale, nodes, leaves, starts, dirs)
    return dict(name=name, scale=scale, nodes=nodes, leaves=leaves, depth=depth, data=data,
                starts=starts, dirs=dirs, w=w, length=3 * 2 ** (depth - 1) + 2)


def device_tree(c, data=True):
    import fourier_feature_nets as ffn
    return ffn.OcTree(float(c["scale"]), c["nodes"], c["leaves"], c["data"] if data else None)


def touched_at(c, rows, t, after=-np.inf):
    """Per ray of ``rows``: is there a leaf whose closed box the ray touches (``t_out == t_in``)
    at exactly ``t``, with ``t > after``?"""
    found = np.zeros(len(rows), bool)
    for leaf_id in c["leaves"]:
        t_in, t_out = closed_touch(c["scale"], leaf_id, c["starts"][rows], c["dirs"][rows])
        found |= (t_in == t_out) & (t_in == t) & (t_in > after)
    return found


# ------------------------------------------------------------------------------------- checks
def check_path(c, w, got_t, got_leaves):
    """The full-length path against the restatement ``w``, t bit for bit.  -> number of deleted
    zero-length stops."""
    length = c["length"]
    hit = w["hit"]
    count = len(hit)
    assert got_t.dtype == np.float32 and got_leaves.dtype == np.int64
    assert got_t.shape == got_leaves.shape == (count, length)
    assert (got_leaves[~hit] == -1).all() and (got_t[~hit] == 0).all()
    assert (got_leaves >= -1).all() and (got_leaves < len(c["leaves"])).all()
    t = got_t[hit].astype(np.float64)
    leaves = got_leaves[hit]
    rows = np.nonzero(hit)[0]
    assert (np.diff(t, axis=1) >= 0).all()
    assert exact(got_t[hit, 0], w["root_in"][hit]) and exact(got_t[hit, -1], w["root_out"][hit])
    assert (leaves[:, -1] == -1).all()
    # no leaf twice in a ray
    ordered = np.sort(leaves, axis=1)
    assert not ((ordered[:, 1:] == ordered[:, :-1]) & (ordered[:, 1:] >= 0)).any()
    # zero-length stops out, the rest to the front
    keep = t[:, 1:] != t[:, :-1]
    order = np.argsort(~keep, axis=1, kind="stable")
    kept = keep.sum(1)
    packed_t = np.take_along_axis(got_t[hit][:, :-1], order, 1)
    packed_l = np.take_along_axis(leaves[:, :-1], order, 1)
    beyond = np.arange(length - 1)[None, :] >= kept[:, None]
    want_t, want_l, written = wref.path(w, length)
    assert (written < length - 1).all()                                  # no cap bites
    assert np.array_equal(kept, written[hit])
    fill = np.repeat(w["root_out"][hit].astype(np.float32)[:, None], length - 1, 1)
    packed_t = np.where(beyond, fill, packed_t)
    packed_l = np.where(beyond, -1, packed_l)
    assert np.array_equal(packed_l, want_l[hit][:, :-1])
    assert exact(packed_t, want_t[hit][:, :-1])
    # every deleted stop is a touch.  (A deleted stop at the cube's exit t without a leaf cannot
    # be told from the fill and needs no telling.)
    gone_r, gone_k = np.nonzero(~keep & (t[:, :-1] < w["root_out"][hit][:, None]) |
                                ~keep & (leaves[:, :-1] >= 0))
    gone_leaf = leaves[gone_r, gone_k]
    at = t[gone_r, gone_k]
    is_leaf = gone_leaf >= 0
    ray = rows[gone_r]
    t_in, t_out = closed_touch(c["scale"], c["leaves"][np.maximum(gone_leaf, 0)][is_leaf],
                               c["starts"][ray[is_leaf]], c["dirs"][ray[is_leaf]])
    assert (t_in == t_out).all() and (t_in == at[is_leaf]).all()
    # an empty region has no number: SOME empty region is touched at that t
    ids, slot, _, _ = wref.regions(c["scale"], c["nodes"], c["leaves"])
    found = np.zeros((~is_leaf).sum(), bool)
    for region in ids[slot < 0]:
        t_in, t_out = closed_touch(c["scale"], region, c["starts"][ray[~is_leaf]],
                                   c["dirs"][ray[~is_leaf]])
        found |= (t_in == t_out) & (t_in == at[~is_leaf])
    assert found.all()
    return len(gone_r)


def check_spans(c, w, t_min, got_in, got_out, got_hit):
    want_in, want_out, want_hit = wref.spans(w, c["scale"], c["depth"], c["dirs"], t_min, 0.0)
    assert got_in.dtype == got_out.dtype == np.float32 and got_hit.dtype == np.bool_
    assert got_hit[want_hit].all()
    assert (got_in[~got_hit] == 0).all() and (got_out[~got_hit] == 0).all()
    g_in, g_out = got_in.astype(np.float64), got_out.astype(np.float64)
    assert (g_in <= want_in)[want_hit].all() and (g_out >= want_out)[want_hit].all()
    # wider than the restatement (or a hit where it has none): the extent ends at a touched leaf
    early = np.nonzero(got_hit & (~want_hit | (g_in < want_in)))[0]
    late = np.nonzero(got_hit & (~want_hit | (g_out > want_out)))[0]
    assert touched_at(c, early, g_in[early], t_min).all()
    assert touched_at(c, late, g_out[late], t_min).all()
    only_touch = got_hit & ~want_hit
    assert (g_in <= g_out)[got_hit].all() and (g_in > t_min)[only_touch].all()
    return len(early), len(late), int(only_touch.sum())


def check_first(c, w, t_min, got_leaf, got_t, got_face):
    """-> number of rays whose first hit is a touched leaf."""
    want = rref.first_hit(w, c["scale"], c["leaves"], c["starts"], c["dirs"], t_min)
    assert got_leaf.dtype == np.int64 and got_t.dtype == np.float32 and got_face.dtype == np.int8
    found = got_leaf >= 0
    assert found[want["leaf"] >= 0].all()
    assert (got_leaf < len(c["leaves"])).all()
    assert (got_t[~found] == 0).all() and (got_face[~found] == -1).all()
    t = got_t.astype(np.float64)
    same = found & (got_leaf == want["leaf"])
    assert exact(got_t[same], want["t"][same])
    touch = np.nonzero(found & ~same)[0]
    t_in, t_out = closed_touch(c["scale"], c["leaves"][got_leaf[touch]], c["starts"][touch],
                               c["dirs"][touch])
    assert (t_in == t_out).all() and (t_in == t[touch]).all() and (t_in > t_min).all()
    later = want["leaf"][touch] >= 0
    assert (t[touch] <= want["t"][touch])[later].all()
    # the face: 6 before t_min, else an axis whose entry plane is crossed at t_hit
    rows = np.nonzero(found)[0]
    centers, depths = oref.leaf_geometry(np.float32(c["scale"]), c["leaves"][got_leaf[rows]])
    half = (np.float64(c["scale"]) / 2.0 ** depths)[:, None]
    o, d = c["starts"][rows].astype(np.float64), c["dirs"][rows].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        near = np.minimum((centers - half - o) / d, (centers + half - o) / d)
    near = np.where(d == 0, -np.inf, near)
    entry = near.max(1)
    clamped = entry < t_min
    face = got_face[rows].astype(np.int64)
    assert (face[clamped] == 6).all() and (face[~clamped] < 6).all() and (face >= 0).all()
    free = np.nonzero(~clamped)[0]
    axis = face[free] >> 1
    assert (near[free, axis] == t[rows][free]).all()
    assert np.array_equal(face[free] & 1, (d[free, axis] < 0).astype(np.int64))
    return len(touch)


def flipped(c):
    """The restatement with the half-open rule of zero components turned round (``lo < o <= hi``):
    a wrong reference."""
    return wref.walk(c["scale"], c["nodes"], c["leaves"], c["starts"], c["dirs"],
                     zero_rule="upper")


def dropped(w, crossing):
    """``w`` without one crossing: a wrong reference."""
    out = dict(w)
    for key in ("ray", "t_in", "t_out", "leaf", "axis_in", "axis_out"):
        out[key] = np.delete(w[key], crossing)
    out["offsets"] = w["offsets"] - (np.arange(len(w["offsets"])) > w["ray"][crossing])
    return out


def wrong_references(c, t_min, leaf_only=True):
    """The two wrong references every comparison is held against: [(what, w)].  The half-open rule
    turned round does not exist in a tree of one region whose only planes are the cube's own."""
    out = [("a dropped region", dropped(c["w"], longest_ray_crossing(c["w"], leaf_only, t_min)))]
    if c["name"] != "root only":
        out.append(("the flipped zero rule", flipped(c)))
    return out


def longest_ray_crossing(w, leaf_only, t_min=0.0):
    """A crossing of positive chord of the ray with the most crossings: its second region, or
    (``leaf_only``) the first leaf of the ray with the most leaves among the rays WITHOUT a tie
    (margin > 0) -- on a ray with ties another leaf may be touched at the very t the dropped one
    began at, and a span or a first hit may begin at a touch."""
    take = (w["leaf"] >= 0) & (w["margin"][w["ray"]] > 0) & (w["t_out"] > t_min) if leaf_only \
        else np.ones(len(w["leaf"]), bool)
    per_ray = np.bincount(w["ray"][take], minlength=len(w["hit"]))
    ray = int(per_ray.argmax())
    mine = np.nonzero((w["ray"] == ray) & take)[0]
    return int(mine[0] if leaf_only else mine[min(1, len(mine) - 1)])


# -------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("name", CASES)
def test_path_equals_the_restatement_on_every_ray(name):
    c = case(name)
    tree = device_tree(c, False)
    path = tree.walk(c["starts"], c["dirs"], c["length"])
    gone = check_path(c, c["w"], path.t_stops, path.leaves)
    print("%s: %d rays (%d hit, %d with margin 0), %d zero-length stops, all touches" %
          (name, len(c["starts"]), c["w"]["hit"].sum(),
           (c["w"]["hit"] & (c["w"]["margin"] == 0)).sum(), gone))
    # a short path: the first max_length - 1 stops of the long one, then the fill
    for short in (3, 6):
        cut = tree.walk(c["starts"], c["dirs"], short)
        assert np.array_equal(bits(cut.t_stops[:, :short - 1]), bits(path.t_stops[:, :short - 1]))
        assert np.array_equal(cut.leaves[:, :short - 1], path.leaves[:, :short - 1])
        assert np.array_equal(bits(cut.t_stops[:, -1]), bits(path.t_stops[:, -1]))
        assert (cut.leaves[:, -1] == -1).all()
    if name == "root only":
        return                                   # one region: no second region to drop
    for what, wrong in wrong_references(c, 0.0, leaf_only=False):
        with pytest.raises(AssertionError):
            check_path(c, wrong, path.t_stops, path.leaves)


@pytest.mark.parametrize("t_min", T_MINS)
@pytest.mark.parametrize("name", CASES)
def test_spans_hold_the_restatement_on_every_ray(name, t_min):
    c = case(name)
    tree = device_tree(c, False)
    got = tree.spans(c["starts"], c["dirs"], t_min, 0.0)
    early, late, only = check_spans(c, c["w"], t_min, *got)
    print("%s t_min=%.2f: %d spans begin and %d end at a touched leaf, %d are touches only" %
          (name, t_min, early, late, only))
    for what, wrong in wrong_references(c, t_min):
        with pytest.raises(AssertionError):
            check_spans(c, wrong, t_min, *got)


@pytest.mark.parametrize("t_min", T_MINS)
@pytest.mark.parametrize("name", CASES)
def test_first_hit_and_render_on_every_ray(name, t_min):
    from fourier_feature_nets_amd import ops
    from tests.test_octree_render_gpu import check_first_hit
    c = case(name)
    w = c["w"]
    tree = device_tree(c)
    hit = tree.first_hit(c["starts"], c["dirs"], t_min)
    touches = check_first(c, w, t_min, hit.leaves, hit.t, hit.faces)
    print("%s t_min=%.2f: %d rays hit a leaf, %d of them a touched one" %
          (name, t_min, (hit.leaves >= 0).sum(), touches))
    # the colour: the leaf's, times the shade of the reported face
    shade = ops.octree_face_shade()
    found = hit.leaves >= 0
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
    # One difference in bits is in the contract: ``first_hit`` returns ``max(entry t, t_min)``,
    # which for an entry at -0 (a plane through the start, crossed with d < 0) and t_min = +0 is
    # +0, while the walk stores the crossing itself.  Nothing else may differ.
    stop_t = path.t_stops[rows, k][free]
    differ = bits(stop_t) != bits(hit.t[free])
    assert (bits(stop_t[differ]) == 0x80000000).all() and (bits(hit.t[free][differ]) == 0).all()
    assert t_min == 0.0 or not differ.any()
    assert (path.t_stops[rows, k][found & ~free] < np.float32(t_min)).all()
    spans = tree.spans(c["starts"], c["dirs"], t_min, 0.0)
    assert np.array_equal(spans[2], found)
    assert np.array_equal(bits(spans[0][found]), bits(hit.t[found]))
    # the rays without any tie, through the checker of the other first-hit tests
    want = rref.first_hit(w, c["scale"], c["leaves"], c["starts"], c["dirs"], t_min)
    plain = ~w["hit"] | (w["margin"] > 0) & (want["edge_gap"] > 0)
    state = dict(scale=c["scale"], node_index=c["nodes"], leaf_index=c["leaves"])
    sub = wref.walk(c["scale"], c["nodes"], c["leaves"], c["starts"][plain], c["dirs"][plain])
    check_first_hit(name + ", no tie", state, c["starts"][plain], c["dirs"][plain], t_min,
                    type(hit)(hit.leaves[plain], hit.t[plain], hit.faces[plain]), sub,
                    every_ray=True)
    for what, wrong in wrong_references(c, t_min):
        with pytest.raises(AssertionError):
            check_first(c, wrong, t_min, hit.leaves, hit.t, hit.faces)


@pytest.mark.parametrize("t_min", T_MINS)
@pytest.mark.parametrize("name", CASES)
def test_volume_on_every_ray(name, t_min):
    from tests.test_octree_volume_gpu import check_volume
    c = case(name)
    tree = device_tree(c)
    state = dict(scale=c["scale"], node_index=c["nodes"], leaf_index=c["leaves"])
    out = tree.render_volume(c["starts"], c["dirs"], t_min, BG)
    check_volume(name, state, c["data"], c["starts"], c["dirs"], t_min, out, c["w"],
                 every_ray=True)
    # the dropped region is an ordinary term: the first leaf of the longest ray without a tie.
    # Between the right and each wrong restatement the colour of some ray differs by at least 2.3
    # budgets on every case here (worked out on the restatements alone).
    for what, wrong in wrong_references(c, t_min):
        with pytest.raises(AssertionError):
            check_volume(name, state, c["data"], c["starts"], c["dirs"], t_min, out, wrong,
                         every_ray=True)


@pytest.mark.parametrize("min_t", [0.0, 1e-3])
@pytest.mark.parametrize("t_min", T_MINS)
@pytest.mark.parametrize("name", CASES)
def test_gradient_on_every_ray(name, t_min, min_t):
    from tests.test_octree_grad_gpu import check_gradient
    c = case(name)
    tree = device_tree(c)
    check_gradient(name, tree, c["data"], c["starts"], c["dirs"], c["w"], t_min, min_t,
                   share=False, every_ray=True)
    # as in the volume test; here some leaf differs by at least 72 budgets between restatements
    for what, wrong in wrong_references(c, t_min):
        with pytest.raises(AssertionError):
            check_gradient(name, tree, c["data"], c["starts"], c["dirs"], wrong, t_min, min_t,
                           share=False, every_ray=True)


@pytest.mark.parametrize("name", CASES)
def test_forward_identity_and_determinism_on_every_ray(name):
    import fourier_feature_nets as ffn
    from tests.test_octree_grad_gpu import cuda, device_gradient, upstream
    c = case(name)
    tree = device_tree(c)
    field = ffn.OctreeField(tree)
    dev_s, dev_d = cuda(c["starts"]), cuda(c["dirs"])
    for t_min, min_t in ((0.0, 0.0), (T_MINS[1], 1e-3)):
        want = tree.render_volume(dev_s, dev_d, t_min, BG, min_t)
        out = field(dev_s, dev_d, t_min, BG, min_t)
        for a, b in zip(out, want):
            assert np.array_equal(bits(a), bits(b))
    d_color, d_alpha = upstream(len(c["starts"]), 6)
    first = device_gradient(tree, c["data"], c["starts"], c["dirs"], d_color, d_alpha, 0.0, BG, 1e-3)
    second = device_gradient(tree, c["data"], c["starts"], c["dirs"], d_color, d_alpha, 0.0, BG, 1e-3)
    assert np.array_equal(bits(first), bits(second))
