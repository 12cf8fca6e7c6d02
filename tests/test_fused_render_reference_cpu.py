"""The float64 reference of the fused render (tests/fused_render_reference.py) checked on its own:
the compacted sequence against the masked full-length one, the teeth, ``keep_of`` on hand-computed
cells, and the proof that the GPU test's case list reaches every branch of the launch arithmetic."""

import types

import pytest
import torch

from tests import composite_reference as cr
from tests import fused_render_reference as fr
from tests import test_fused_render_reference_gpu as cases

CUS = 256          # the plan takes the CU count as a parameter; the GPU test reads the device's


def _masks(R, S, seed):
    gen = torch.Generator().manual_seed(seed)
    out = dict(bern05=torch.rand(R, S, generator=gen) < 0.5, bern01=torch.rand(R, S, generator=gen) < 0.1)
    for name in ("none", "all", "first", "last", "second_last", "all_but_last", "even", "odd", "first33",
                 "runs", "runs_b"):
        out[name] = cases.pattern_row(name, S, 0)[None].repeat(R, 1)
    return out


def _close(a, b):
    return bool(((a - b).abs() <= 1e-12 * torch.maximum(a.abs(), b.abs())).all())


@pytest.mark.parametrize("S", [1, 2, 33, 64, 65, 130])
def test_compacted_equals_masked(S):
    """Two float64 evaluations of one quantity: the compacted sequence, and the full-length K5
    reference with sigma := 0 exactly at the skipped samples.  Every regime of ``make_rays``."""
    R = 3 * len(cr.REGIMES)
    logits, t, _ = cr.make_rays(R, S, S)
    for name, keep in _masks(R, S, S).items():
        a = fr.render_reference(logits, t, keep)
        b = fr.masked_reference(logits, t, keep)
        assert _close(a["colour"].v, b["colour"].v), name
        assert _close(a["alpha"].v, b["alpha"].v), name
        assert _close(a["weights"].v, torch.where(keep, b["weights"].v, 0.0)), name
        assert bool((a["candidates"] & b["candidates"]).any(1).all()), name
        # the budget counts the kept samples only: never more than the full-length budget
        assert bool((a["colour"].b <= b["colour"].b * (1 + 1e-12)).all()), name
        assert torch.equal(a["m"], keep.sum(1))
    empty = fr.render_reference(logits, t, torch.zeros(R, S, dtype=torch.bool))
    assert float(empty["colour"].v.abs().max()) == 0.0 and float(empty["alpha"].v.abs().max()) == 0.0
    only_last = torch.arange(S)[None] == S - 1
    assert torch.equal(empty["candidates"], only_last.expand(R, S))          # depth t[S - 1]


@pytest.mark.parametrize("S", [1, 2, 64, 65, 130])
def test_without_a_grid_it_is_the_k5_reference(S):
    logits, t, _ = cr.make_rays(14, S, 3)
    a = fr.render_reference(logits, t)
    b = cr.composite_forward(logits, t)
    for out in ("colour", "alpha"):
        assert torch.equal(a[out].v, b[out].v) and torch.equal(a[out].b, b[out].b)
    assert torch.equal(a["weights"].v, b["wt"]["w"].v) and torch.equal(a["weights"].b, b["wt"]["w"].b)
    assert torch.equal(a["candidates"], cr.depth_candidates(b))


def _constructed(S=100, R=8):
    """Moderate density (alpha sums well above 0.1, weights that matter all along the ray)."""
    gen = torch.Generator().manual_seed(11)
    logits = torch.randn(R, S, 4, generator=gen)
    logits[..., 3] = 0.5 + 0.5 * torch.randn(R, S, generator=gen)
    t = (torch.linspace(0.0, 2.0, S)[None] + 0.01 * torch.rand(R, 1, generator=gen)).float().contiguous()
    names = ["runs", "runs_b", "bern0.5", "odd", "first33", "all_but_last", "bern0.9", "even"]
    keep = cases.keep_rows(names[:R], S)
    return logits, t, keep


@pytest.mark.parametrize("tooth", fr.TEETH)
def test_teeth_bite(tooth):
    """Each changed reference moves colour or alpha beyond the bound of some constructed ray
    (``slot_depth``: its candidates miss every candidate of the reference on some ray)."""
    logits, t, keep = _constructed()
    ref = fr.render_reference(logits, t, keep)
    alt = fr.render_reference(logits, t, keep, tooth)
    if tooth == "slot_depth":
        assert torch.equal(alt["colour"].v, ref["colour"].v)
        assert bool((~(ref["candidates"] & alt["candidates"]).any(1)).any())
        return
    moved = False
    for out in ("colour", "alpha"):
        bound = fr.KAPPA[out] * fr.U * ref[out].b
        moved = moved or bool(((alt[out].v - ref[out].v).abs() > bound).any())
    assert moved


def test_the_gpu_cases_reach_every_branch_of_the_plan():
    seen = dict(rounds=set(), ragged=set(), nblk=set(), m=set(), pairs=set(), tail=set(), rows=set())
    for label, R, S, teams, names in cases.plan_cases(CUS):
        plan = fr.render_plan(R, S, teams, CUS)
        wide = teams == fr.WIDE_TEAMS
        assert plan["wide"] == wide and plan["grid"] <= CUS
        assert plan["rays_per_round"] * plan["rounds"] - plan["idle_teams"] == R
        seen["rounds"].add((wide, min(plan["rounds"], 2)))
        seen["ragged"].add((wide, plan["ragged"]))
        # every ray has its own place in the launch
        if R < 5000:
            places = {fr.ray_place(r, plan) for r in range(R)}
            assert len(places) == R and max(p[0] for p in places) == plan["rounds"] - 1
            assert max(p[1] for p in places) < plan["grid"]
        if names is None:
            continue
        keep = cases.keep_rows(names, S)
        valid = torch.tensor([n != "invalid" for n in names])
        m = (keep & valid[:, None]).sum(1).tolist()
        for r, mr in enumerate(m):
            ray = fr.render_plan(R, S, teams, CUS, mr)
            assert ray["nblk"] * 32 - ray["tail_lanes"] == mr and ray["rows"] == -(-mr // 64)
            seen["nblk"].add(ray["nblk"])
            seen["rows"].add(ray["rows"])
            seen["m"].add((S, mr))
            seen["tail"].add(ray["tail_lanes"] > 0)
            if wide and r % 2 == 0 and r + 1 < R:
                assert fr.ray_place(r, plan)[:2] == fr.ray_place(r + 1, plan)[:2]
                pair = fr.pair_plan(mr, m[r + 1])
                seen["pairs"].add((pair["dummy"][0] > 0, pair["dummy"][1] > 0,
                                   0 in pair["nblk"] and pair["passes"] == -(-S // 32)))
    for wide in (False, True):
        assert (wide, 1) in seen["rounds"] and (wide, 2) in seen["rounds"]
        assert (wide, True) in seen["ragged"]                  # R mod teams != 0
    assert (False, False) in seen["ragged"]
    assert {0, 1, 2, 3, 4, 7, 8} <= seen["nblk"]               # none, one, two, odd and even, the most
    assert {0, 1, 2, 4} <= seen["rows"] and seen["tail"] == {True, False}
    for S in cases.COMPACT_S:
        for want in (0, 1, 31, 32, 33, 63, 64, 65, S - 1, S):
            if want <= S:
                assert (S, want) in seen["m"], (S, want)
    # wide pairs: the left pair pads, the right pair pads, and nothing against the most there is
    assert (True, False, True) in seen["pairs"] and (False, True, True) in seen["pairs"]
    assert (False, False, False) in seen["pairs"]
    # patterns whose names promise something
    for S in (65, 200, 256):
        row = cases.pattern_row("runs", S, 0)
        slots = torch.cumsum(row.long(), 0) - 1                 # slot of a kept sample
        for edge in (32, 64):
            if int(row.sum()) > edge:
                j = int((row & (slots == edge)).nonzero()[0, 0])
                run = row[:j + 1].flip(0).long().cumprod(0).sum()     # kept samples ending at j
                assert 1 < int(run) <= int(slots[j]), (S, edge)       # inside a run that began after a skip
        assert not bool(row[S - 1])
        other = cases.pattern_row("runs_b", S, 0)
        assert not bool(other[0]) and (S < 200 or bool(other[S - 1]))
    for S in cases.COMPACT_S + cases.WIDE_S + [cases.LIST_S] + cases.NO_GRID_S:
        ix = cases.sample_cells(S)
        assert len(set(ix.tolist())) == S and 0 <= int(ix.min()) and int(ix.max()) < cases.G


def test_keep_of_on_hand_computed_cells():
    g = 4
    cells = torch.tensor([0, 57, 63])          # (0,0,0), (1,2,3) = (3*4 + 2)*4 + 1, (3,3,3)
    bits = fr.grid_bits(cells, g)
    assert bits.dtype == torch.int32 and bits.tolist() == [1, (1 << 25) + (1 << 31) - (1 << 32)]
    grid = types.SimpleNamespace(bits=bits, box_min=[-1.0, -1.0, -1.0], box_size=[2.0, 2.0, 2.0], resolution=g)
    nan = float("nan")
    points = torch.tensor([[-0.9, -0.9, -0.9],      # cell (0,0,0)
                           [0.9, 0.9, 0.9],         # (3,3,3)
                           [-0.25, 0.25, 0.75],     # (1,2,3), every coordinate in the middle of its cell
                           [0.25, 0.25, 0.75],      # (2,2,3): empty
                           [1.0, 1.0, 1.0],         # on the far faces: clamped into (3,3,3)
                           [-1.5, -1.0, -1.25],     # outside: clamped into (0,0,0)
                           [1.5, 0.25, 0.75],       # outside: clamped into (3,2,3), empty
                           [nan, 0.0, 0.0],         # NaN: occupied
                           [0.25, nan, 0.75]])
    keep, dist = fr.keep_of(points, grid)
    assert keep.tolist() == [True, True, True, False, True, True, False, True, True]
    assert torch.allclose(dist[2], torch.tensor([0.5, 0.5, 0.5], dtype=torch.float64))
    assert float(dist[4].max()) == 0.0 and abs(float(dist[0, 0]) - 0.2) < 1e-6
    assert bool(torch.isnan(dist[7, 0])) and float(dist[5, 1]) == 0.0
    # a coordinate that rounds: fl(fl(x - min) * inv), both roundings in f32
    x = torch.tensor([[0.1, 0.0, 0.0]])
    grid3 = types.SimpleNamespace(bits=fr.grid_bits(torch.tensor([0]), 3), box_min=[0.1, -1.0, -1.0],
                                  box_size=[0.3, 2.0, 2.0], resolution=3)
    f32 = torch.float32
    inv = torch.tensor(3.0, dtype=f32) / torch.tensor(0.3, dtype=f32)
    want = ((x[0, 0] - torch.tensor(0.1, dtype=f32)) * inv).double()
    _, d = fr.keep_of(x, grid3)
    assert float(d[0, 0]) == float(torch.minimum(want - want.floor(), 1 - (want - want.floor())))
