"""The helpers behind tests/test_data_parallel_gpu.py on their own (no GPU): the shard bounds
restated from `TrainEngine.shard`, the cutter of the per-step noise block, and the `max_samples`
rule that makes one process launch exactly the shards of `world` ranks."""

import inspect

import pytest
import torch

from tests import dp_worker

SIZES = [(n, world) for n in range(11) for world in range(1, 5)]


@pytest.mark.parametrize("n,world", SIZES)
def test_shard_bounds_tile_the_batch(n, world):
    bounds = dp_worker.shard_bounds(n, world)
    assert len(bounds) == world and bounds[0][0] == 0 and bounds[-1][1] == n
    assert all(a[1] == b[0] for a, b in zip(bounds, bounds[1:]))          # contiguous, in rank order
    per = -(-n // world)
    sizes = [hi - lo for lo, hi in bounds]
    # full shards, at most one short one, then empty ones: trailing ranks of a tiny batch get nothing
    full, rest = divmod(n, per) if per else (0, 0)
    assert sizes == [per] * full + ([rest] if rest else []) + [0] * (world - full - (1 if rest else 0))
    # ... which is what the slices of the product's `shard` select
    rays = torch.arange(100, 100 + n)
    for rank, (lo, hi) in enumerate(bounds):
        assert torch.equal(rays[rank * per:(rank + 1) * per], rays[lo:hi])


def test_shard_bounds_restate_the_products_rule():
    """The two lines the restatement stands for are still the product's."""
    from fourier_feature_nets_amd.caster import TrainEngine
    source = inspect.getsource(TrainEngine.shard)
    assert "per = -(-rays.numel() // world)" in source
    assert "rays[rank * per:(rank + 1) * per]" in source
    source = inspect.getsource(TrainEngine.train_step)
    assert "per_launch = max(1, self.max_samples // sampler.num_samples)" in source
    assert "for lo in range(0, count, per_launch):" in source


def test_empty_trailing_shards_where_expected():
    assert dp_worker.shard_bounds(4, 3) == [(0, 2), (2, 4), (4, 4)]
    assert dp_worker.shard_bounds(1, 3) == [(0, 1), (1, 1), (1, 1)]
    assert dp_worker.shard_bounds(3, 3) == [(0, 1), (1, 2), (2, 3)]
    assert dp_worker.shard_bounds(0, 2) == [(0, 0), (0, 0)]
    assert dp_worker.shard_bounds(9, 4) == [(0, 3), (3, 6), (6, 9), (9, 9)]


@pytest.mark.parametrize("n,world", SIZES)
@pytest.mark.parametrize("num_samples", [1, 16])
def test_reference_launches_are_the_non_empty_shards(n, world, num_samples):
    limit = dp_worker.reference_max_samples(n, world, num_samples)
    launches = dp_worker.launch_bounds(n, limit, num_samples)
    assert launches == [b for b in dp_worker.shard_bounds(n, world) if b[1] > b[0]]
    if len(launches) >= 2:
        # the controls: one ray more per launch is another cut
        assert dp_worker.launch_bounds(n, limit + num_samples, num_samples) != launches


@pytest.mark.parametrize("n,world", SIZES)
@pytest.mark.parametrize("widths", [(), (16,), (8, 8), (3, 4)])
def test_noise_cutter_hands_out_every_row_exactly_once(n, world, widths):
    columns = sum(widths)
    block = torch.arange(n * columns, dtype=torch.float32).reshape(n, columns)      # every entry unique
    shards = dp_worker.shard_bounds(n, world)
    per_rank = [dp_worker.cut_noise(block, [shards[rank]], widths) for rank in range(world)]
    for (lo, hi), pieces in zip(shards, per_rank):
        assert len(pieces) == (len(widths) if hi > lo else 0)
        assert [tuple(p.shape) for p in pieces] == [(hi - lo, w) for w in widths if hi > lo]
    if widths:
        rows = [torch.cat(pieces, dim=1) for pieces in per_rank if pieces]
        together = torch.cat(rows) if rows else block[:0]
        assert torch.equal(together, block)                     # each row once, in order, nothing else
    # the one-process reference draws the ranks' pieces in rank order
    reference = dp_worker.cut_noise(block, shards, widths)
    ranks = [p for pieces in per_rank for p in pieces]
    assert len(reference) == len(ranks) and all(torch.equal(a, b) for a, b in zip(reference, ranks))


def test_noise_widths_follow_the_samplers_draws():
    assert dp_worker.noise_widths(16, False, "table") == ()
    assert dp_worker.noise_widths(16, True, None) == (16,)
    assert dp_worker.noise_widths(16, True, "live") == (8, 8)
    assert dp_worker.noise_widths(15, True, "table") == (7, 8)


def test_noise_feed_refuses_an_unplanned_or_mis_shaped_draw():
    feed = dp_worker.NoiseFeed("cpu")
    feed.push([torch.zeros(3, 8), torch.ones(3, 8)])
    assert feed(3, 8).sum() == 0 and feed.calls == 1
    with pytest.raises(AssertionError):
        feed(2, 8)                                             # (the piece is consumed: a test fails here)
    with pytest.raises(AssertionError, match="unplanned"):
        feed(3, 8)
    assert feed.calls == 3


def test_scenario_table():
    assert sorted(dp_worker.SCENARIOS) == ["empty-shard", "nerf-bf16x6", "nerf-live", "nerf-table",
                                           "no-rays", "wide-occupancy"]
    for name, spec in dp_worker.SCENARIOS.items():
        assert spec["world"] == (3 if name == "empty-shard" else 2)
        assert len(spec.get("counts", (None,) * dp_worker.STEPS)) == dp_worker.STEPS
    assert dp_worker.STEPS == 3 and dp_worker.LEARNING_RATE == 5e-4
