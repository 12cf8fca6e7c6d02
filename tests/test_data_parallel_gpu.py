"""Data-parallel training steps on the model / sampler combinations of the multi-GPU
configurations (BASELINE config 4: full NeRF chain with view directions, stratified jitter and
opacity-guided focus samples; config 5: 512-wide Gaussian features with occupancy compaction), on
empty shards and on a batch without a valid ray -- held to a one-process run EXACTLY.

The reference is the product's own `train_step` with `max_samples` set to one shard's sample
count: its launches are then the shards of the ranks, and `grads.add_(part)` is the one f32
addition a two-rank all-reduce performs (tests/dp_worker.py, "scenarios").  Addition of two f32
values is commutative, so ranks and reference must agree bit for bit; nothing here rests on a
tolerance except the one step of `empty-shard` that sums three contributions.  That the chunked
step equals the single-launch step is `test_micro_batched_step_equals_single_launch`'s business.

Two conditions keep the comparison exact and are asserted with every scenario, so that a
violation is not read as a product bug: every rank does exactly one launch per step, and the
reference's launches are the shards.  Two controls show that the comparison can fail."""

import contextlib
import io
import math
import os
import socket
import time

import numpy as np
import pytest
import torch

from tests import dp_worker

pytestmark = pytest.mark.gpu

DEADLINE_S = 300.0
STATE = ("flat", "exp_avg", "exp_avg_sq", "grad_norm")


def dev():
    return torch.device("cuda:0")


def _free_port():
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        return sock.getsockname()[1]


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    """The 20 + 10 camera 128x128 rig of the config-3 fixture, written once for every process."""
    from tests.golden.make_fit_schedule_nerf import SIZE, TRAIN_CAMS, VAL_CAMS
    from tests.psnr_ensemble import write_npz
    return write_npz(str(tmp_path_factory.mktemp("dp_scene") / "scene.npz"), TRAIN_CAMS, VAL_CAMS, SIZE)


def _spawn(world, names, scene, out_dir):
    """`world` ranks through every scenario of `names` in ONE spawn, joined against a deadline:
    on the deadline (or a rank's failure) the children are terminated and the caller fails.
    Returns ({scenario: [rank 0's result, rank 1's, ...]}, wall seconds)."""
    import torch.multiprocessing as mp
    began = time.monotonic()
    ctx = mp.start_processes(dp_worker.dp_scenarios_worker,
                             args=(world, _free_port(), out_dir, names, scene),
                             nprocs=world, join=False, start_method="spawn")
    try:
        while True:
            left = DEADLINE_S - (time.monotonic() - began)
            if left <= 0:
                raise TimeoutError("%d ranks did not finish %s within %.0f s" % (world, names, DEADLINE_S))
            if ctx.join(timeout=left):
                break
    finally:
        for proc in ctx.processes:
            if proc.is_alive():
                proc.terminate()
        for proc in ctx.processes:
            proc.join(10)
    results = {name: [torch.load(os.path.join(out_dir, "%s.%d.pt" % (name, rank)), weights_only=False)
                      for rank in range(world)] for name in names}
    return results, time.monotonic() - began


@pytest.fixture(scope="module")
def ranks(tmp_path_factory, scene):
    """Every scenario's per-rank results: one spawn per world size for the whole module."""
    out = {}
    for world in sorted({spec["world"] for spec in dp_worker.SCENARIOS.values()}):
        names = [name for name, spec in dp_worker.SCENARIOS.items() if spec["world"] == world]
        results, seconds = _spawn(world, names, scene, str(tmp_path_factory.mktemp("dp_ranks%d" % world)))
        print("data parallel: %d ranks x %s took %.1f s" % (world, names, seconds))
        out.update(results)
    return out


_REFERENCES = {}


def _reference(name, scene):
    """The one-process run of a scenario, computed once and left unchanged."""
    if name not in _REFERENCES:
        _REFERENCES[name] = dp_worker.run_scenario(name, None, dp_worker.SCENARIOS[name]["world"], scene)
    return _REFERENCES[name]


def _same(a, b):
    """Equal by value (`torch.equal`: -0 and +0 are equal); NaN equals NaN only for a loss."""
    return torch.equal(a, b) or bool(a.ndim == 0 and torch.isnan(a) and torch.isnan(b))


def _first_difference(mine, theirs, steps):
    """The first (step, quantity) at which two runs differ, or None."""
    for step in steps:
        for key in ("loss",) + STATE:
            if not _same(mine["steps"][step][key], theirs["steps"][step][key]):
                return step, key
        if mine["steps"][step]["count"] != theirs["steps"][step]["count"]:
            return step, "count"
    return None


def _expect_prefetch(spec, counts, rank, step):
    """Whether `rank` must hold a look-ahead after `step`: the scenario's sampler may be drawn
    ahead, another step follows, and the rank's shard of it is not empty."""
    if not spec["prefetch"] or step + 1 >= len(counts):
        return False
    lo, hi = dp_worker.shard_bounds(counts[step + 1], spec["world"])[rank]
    return hi > lo


def _check_scenario(name, ranks, reference):
    """Everything a scenario asserts; `exact_steps` are compared bit for bit."""
    spec = dp_worker.SCENARIOS[name]
    world = spec["world"]
    mine = ranks[name]
    if "refused" in reference:
        # the mode has no kernels for this chain: every rank and the reference refused the step
        assert all(r == {"refused": True} for r in mine) and reference == {"refused": True}
        return
    counts = reference["counts"]
    steps = range(dp_worker.STEPS)
    widths = reference["noise_widths"]
    for r in mine:
        assert r["counts"] == counts and r["noise_widths"] == widths
    print("%s: global counts %s" % (name, counts))

    # -- the two conditions of exactness
    for step in steps:
        shards = dp_worker.shard_bounds(counts[step], world)
        filled = [b for b in shards if b[1] > b[0]]
        # (the reference's launch boundaries are the shard boundaries ...)
        assert reference["planned"][step] == filled, (step, reference["planned"][step], shards)
        ref_chunks = [c["rays"] for c in reference["chunks"] if c["step"] == step]
        assert all(c["during"] == c["step"] for c in reference["chunks"])
        rank_chunks = []
        for rank, r in enumerate(mine):
            own = [c for c in r["chunks"] if c["step"] == step]
            lo, hi = shards[rank]
            # (... and every rank does exactly one launch per step, none on an empty shard)
            assert len(own) == (1 if hi > lo else 0), (step, rank, len(own))
            assert r["planned"][step] == ([shards[rank]] if hi > lo else [])
            rank_chunks += [c["rays"] for c in own]
        assert len(ref_chunks) == len(rank_chunks) == len(filled)
        for a, b, (lo, hi) in zip(ref_chunks, rank_chunks, filled):
            assert a.numel() == hi - lo and torch.equal(a, b), step
    shard_sizes = [[hi - lo for lo, hi in dp_worker.shard_bounds(n, world)] for n in counts]
    print("%s: shard sizes %s" % (name, shard_sizes))

    # -- sampling ahead of the optimiser update: used where allowed, refused elsewhere
    stored = []
    for rank, r in enumerate(mine):
        assert r["can_prefetch"] == spec["prefetch"]
        for step in steps:
            expected = _expect_prefetch(spec, counts, rank, step)
            assert r["steps"][step]["prefetched"] == expected, (rank, step)
            own = [c for c in r["chunks"] if c["step"] == step]
            if step > 0 and _expect_prefetch(spec, counts, rank, step - 1):
                # the samples of this step were drawn during the step before, and used: this step
                # itself sampled nothing
                assert [c["during"] for c in own] == [step - 1], (rank, step)
            else:
                assert all(c["during"] == step for c in own), (rank, step)
        stored.append(sum(r["steps"][step]["prefetched"] for step in steps))
    assert not reference["can_prefetch"] or spec["prefetch"]
    assert not any(s["prefetched"] for s in reference["steps"])      # (announced to ranks only)
    print("%s: look-aheads stored per rank %s" % (name, stored))

    # -- no silent extra draw: the `_noise` calls of every step are the planned ones
    for rank, r in enumerate(mine + [reference]):
        for step in steps:
            if r is reference:
                sampled = len(r["planned"][step])
            else:
                sampled = sum(1 for c in r["chunks"] if c["during"] == step)
            assert r["steps"][step]["noise_calls"] == sampled * len(widths), (rank, step)

    # -- occupancy compaction: part of the volume, another count on every rank
    if spec.get("occupancy"):
        for r in mine + [reference]:
            for step in steps:
                assert 0.0 < r["steps"][step]["fraction"] < 1.0
        kept = [[[m for _, m in r["steps"][step]["compacted"]] for r in mine] for step in steps]
        print("%s: compacted samples per step and rank %s of %s" % (
            name, kept, [[n for n, _ in reference["steps"][step]["compacted"]] for step in steps]))
        assert any(a != b for (a,), (b,) in kept)
        for step in steps:        # the reference compacted the same samples, launch by launch
            got = [c for r in mine for c in r["steps"][step]["compacted"]]
            assert got == reference["steps"][step]["compacted"], step
    else:
        assert all(s["fraction"] is None for r in mine for s in r["steps"])

    # -- ranks in lockstep with each other, on every step (tolerance steps included)
    for rank in range(1, world):
        assert _first_difference(mine[0], mine[rank], steps) is None, rank

    # -- and equal to the reference, bit for bit
    exact = [step for step in steps
             if sum(1 for lo, hi in dp_worker.shard_bounds(counts[step], world) if hi > lo) <= 2]
    if len(exact) < len(steps):
        # only `empty-shard` has such a step, and it is its last: three contributions meet in the
        # all-reduce, (a + b) + c against whatever order gloo takes
        assert name == "empty-shard" and exact == [0, 1]
    assert _first_difference(mine[0], reference, exact) is None, _first_difference(mine[0], reference, exact)
    for step in steps:
        if step not in exact:
            # the project's tolerance on the loss (test_two_rank_train_step_equals_one_rank); the
            # weights after this step are NOT compared
            np.testing.assert_allclose(float(mine[0]["steps"][step]["loss"]),
                                       float(reference["steps"][step]["loss"]), rtol=2e-6)
    assert min(r["moved"] for r in mine) > 1e-4          # the weights did move
    return mine, reference


@pytest.mark.parametrize("name", ["nerf-table", "nerf-live", "nerf-bf16x6", "wide-occupancy"])
def test_sharded_steps_equal_the_chunked_one_process_steps(name, ranks, scene):
    """Two ranks, three annealed steps on ragged every-third-ray batches: losses, weights, both
    Adam moments and the gradient norm of every step equal the one-process run whose launches are
    the two shards."""
    reference = _reference(name, scene)
    _check_scenario(name, ranks, reference)
    if name == "nerf-bf16x6" and "refused" not in reference and os.environ.get("FFN_PRECISION", "f32") == "f32":
        # (the mode did change the arithmetic: otherwise this is `nerf-table` twice -- as it is
        # when the whole suite runs under --precision bf16x6)
        table = _reference("nerf-table", scene)
        assert _first_difference(reference, table, range(dp_worker.STEPS)) is not None


def test_empty_shards_contribute_exactly_nothing(ranks, scene):
    """Three ranks on batches of 4, 1 and 3 valid rays: shards (2,2,0), (1,0,0) and (1,1,1).  The
    steps whose third shard is empty are compared exactly (an empty shard's reduce buffer is
    exactly zero, so the order of the three-way sum cannot matter).  The (1,1,1) step is last and
    only its loss is compared, at the project's rtol = 2e-6: (a + b) + c is not a + (b + c), and
    the weights it leaves are not compared."""
    reference = _reference("empty-shard", scene)
    mine, _ = _check_scenario("empty-shard", ranks, reference)
    assert reference["counts"] == [4, 1, 3]
    assert [len(p) for p in reference["planned"]] == [2, 1, 3]
    assert [[len(r["planned"][step]) for r in mine] for step in range(3)] == [[1, 1, 0], [1, 0, 0], [1, 1, 1]]


def test_a_batch_without_a_valid_ray_skips_the_step_on_every_rank(ranks, scene):
    """An empty int64 `rays=` between two ordinary steps: every rank reports a NaN loss, the step
    count, the weights and both moments keep their bits, and the step after it equals the
    reference's."""
    reference = _reference("no-rays", scene)
    mine, _ = _check_scenario("no-rays", ranks, reference)
    assert reference["counts"][1] == 0 and min(reference["counts"][0], reference["counts"][2]) > 2
    for r in mine + [reference]:
        before, skipped, after = r["steps"]
        assert math.isnan(float(skipped["loss"])) and math.isfinite(float(after["loss"]))
        assert before["count"] == skipped["count"] == 1 and after["count"] == 2
        for key in ("flat", "exp_avg", "exp_avg_sq"):
            # (bit-unchanged: not even a zero's sign may flip)
            assert torch.equal(before[key].view(torch.int32), skipped[key].view(torch.int32)), key
            assert not torch.equal(skipped[key], after[key]), key


# ----------------------------------------------------------------------------------- controls
def test_controls_a_wrong_shard_cut_or_a_lost_shard_is_not_equal(ranks, scene):
    """If either of these passed as equal, the module would prove nothing: a reference whose
    launches are cut ONE ray off the shard boundary, and one that drops the second launch, do not
    reproduce the ranks' `nerf-table` result."""
    mine = ranks["nerf-table"][0]
    steps = range(dp_worker.STEPS)
    assert _first_difference(mine, _reference("nerf-table", scene), steps) is None
    world = dp_worker.SCENARIOS["nerf-table"]["world"]
    shifted = dp_worker.run_scenario("nerf-table", None, world, scene, shift=1)
    n = shifted["counts"][0]
    lo, hi = dp_worker.shard_bounds(n, world)[0]
    assert shifted["planned"][0] == [(0, hi + 1), (hi + 1, n)]
    found = _first_difference(mine, shifted, steps)
    print("control, cut one ray off: first difference", found)
    assert found is not None
    dropped = dp_worker.run_scenario("nerf-table", None, world, scene, drop_second=True)
    assert dropped["planned"][0] == [(lo, hi)]
    found = _first_difference(mine, dropped, steps)
    print("control, second launch dropped: first difference", found)
    assert found is not None and found[0] == 0


# ----------------------------------------------------------------------------------- one-rank RCCL group
NUM_STEPS, FIT_BATCH = 4, 1024


def _fit_nerf(scene, focus_mode, use_group, crop_steps=0, num_steps=NUM_STEPS):
    """`Raycaster.fit` on the NeRF fixture with stratified jitter from the DEVICE generator,
    optionally over a one-rank nccl (= RCCL) group: the asynchronous all-reduce with the next
    step's sampling enqueued under it.  `num_steps` stays inside one epoch (320 batches of
    FIT_BATCH rays), so every announced batch is consumed unless the crop is removed."""
    import torch.distributed as dist
    import fourier_feature_nets_amd as ffn
    model = dp_worker._nerf_model(dev())
    train, val = dp_worker.nerf_datasets(scene, focus_mode, dev(), True, with_val=True)
    assert train.sampler.noise_source == "device" and train.sampler.stratified
    torch.manual_seed(777)
    np.random.seed(777)
    caster = ffn.Raycaster(model)
    record = {"given": [], "samples": [], "stored": [], "prefetch_calls": 0, "after": []}
    current = [None]
    orig_step, orig_samples, orig_prefetch = (ffn.TrainEngine.train_step, ffn.TrainEngine._samples,
                                              ffn.TrainEngine._prefetch)

    def recording_step(self, dataset, batch, step, lr, rays=None, lookahead=None):
        current[0] = step
        record["given"].append(rays.detach().cpu().clone())
        out = orig_step(self, dataset, batch, step, lr, rays=rays, lookahead=lookahead)
        record["after"].append(getattr(self, "_prefetched", None) is not None)
        return out

    def recording_samples(self, sampler, chunk, step):
        out = orig_samples(self, sampler, chunk, step)
        if sampler is train.sampler:
            record["samples"].append({"during": current[0], "step": step, "rays": chunk.detach().cpu().clone(),
                                      "t": out[0].detach().cpu().clone()})
        return out

    def counting_prefetch(self, lookahead):
        record["prefetch_calls"] += 1
        orig_prefetch(self, lookahead)
        if getattr(self, "_prefetched", None) is not None:
            record["stored"].append(lookahead[2])

    if use_group:
        dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % _free_port(), rank=0,
                                world_size=1, device_id=dev())
        caster.process_group = dist.group.WORLD
    ffn.TrainEngine.train_step, ffn.TrainEngine._samples = recording_step, recording_samples
    ffn.TrainEngine._prefetch = counting_prefetch
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            caster.fit(train, val, FIT_BATCH, 5e-4, num_steps, crop_steps, 5, 0.1, 25000, 0.0, [])
        assert not caster.engine._host_staged
        caster.engine.check_finite()
    finally:
        ffn.TrainEngine.train_step, ffn.TrainEngine._samples = orig_step, orig_samples
        ffn.TrainEngine._prefetch = orig_prefetch
        if use_group:
            dist.destroy_process_group()
    record["flat"] = caster.engine.flat.detach().cpu().clone()
    record["engine"] = caster.engine
    return record


def test_rccl_fit_draws_the_next_steps_samples_under_the_all_reduce(scene):
    """Table focus, device noise, no crop: over the one-rank RCCL group a look-ahead is stored for
    every step but the last and USED (each later step samples nothing itself); the t-values handed
    to every step and the final weights equal the group-less run bit for bit -- nothing else draws
    from the device generator between the end of step k and the start of step k + 1."""
    alone = _fit_nerf(scene, "table", False)
    group = _fit_nerf(scene, "table", True)
    assert alone["prefetch_calls"] == 0 and alone["stored"] == []
    assert [s["during"] for s in alone["samples"]] == list(range(NUM_STEPS + 1))
    assert group["stored"] == list(range(1, NUM_STEPS + 1))
    assert group["after"] == [True] * NUM_STEPS + [False]
    assert [(s["during"], s["step"]) for s in group["samples"]] == \
        [(0, 0)] + [(step - 1, step) for step in range(1, NUM_STEPS + 1)]
    print("rccl fit, table focus: look-aheads stored for steps", group["stored"])
    assert len(alone["given"]) == len(group["given"]) == NUM_STEPS + 1
    for step in range(NUM_STEPS + 1):
        assert torch.equal(alone["given"][step], group["given"][step]), step
        a, b = alone["samples"][step], group["samples"][step]
        assert a["step"] == b["step"] == step and torch.equal(a["rays"], group["given"][step])
        assert torch.equal(a["rays"], b["rays"]) and torch.equal(a["t"], b["t"]), step
    assert not torch.equal(alone["samples"][0]["t"][:64], alone["samples"][1]["t"][:64])
    assert torch.equal(alone["flat"], group["flat"])


def test_rccl_fit_never_draws_ahead_of_a_live_coarse_pass(scene):
    """The same with `focus_mode="live"`: every announcement is refused (`_can_prefetch`), no
    look-ahead is ever stored, and the weights equal the group-less run's."""
    alone = _fit_nerf(scene, "live", False)
    group = _fit_nerf(scene, "live", True)
    assert group["prefetch_calls"] == NUM_STEPS and group["stored"] == []
    assert group["after"] == [False] * (NUM_STEPS + 1)
    assert [(s["during"], s["step"]) for s in group["samples"]] == [(k, k) for k in range(NUM_STEPS + 1)]
    for a, b in zip(alone["samples"], group["samples"]):
        assert torch.equal(a["rays"], b["rays"]) and torch.equal(a["t"], b["t"])
    assert torch.equal(alone["flat"], group["flat"])


def test_rccl_fit_discards_the_look_ahead_at_crop_removal(scene):
    """Crop removal inside the run (`crop_steps=2`, three steps after step 0): the batch announced
    during step 2 belongs to the cropped epoch and is never trained on.  The discarded draw shifts
    the device generator, which `fit` accepts, so nothing is compared with the group-less run;
    what must hold is that step 3 sampled the rays it was GIVEN, not the announced ones, and that
    no look-ahead is left behind."""
    group = _fit_nerf(scene, "table", True, crop_steps=2, num_steps=3)
    assert group["stored"] == [1, 2, 3] and group["after"] == [True, True, True, False]
    for_step_3 = [s for s in group["samples"] if s["step"] == 3]
    assert [s["during"] for s in for_step_3] == [2, 3]
    announced, sampled = for_step_3
    given = group["given"][3]
    assert torch.equal(sampled["rays"], given)                    # (world 1: the shard is the batch)
    assert not (announced["rays"].numel() == given.numel() and torch.equal(announced["rays"], given))
    assert [(s["during"], s["step"]) for s in group["samples"] if s["step"] < 3] == [(0, 0), (0, 1), (1, 2)]
    assert getattr(group["engine"], "_prefetched", None) is None
