"""Worker bodies of the multi-process GPU tests (spawned with torch.multiprocessing, so they
must live in an importable module).  Every rank drives the PRODUCT's TrainEngine.train_step on
cuda:0 (ranks share the one GPU of the test box) over a gloo group, which the engine reduces
through the host."""

import contextlib
import io
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SCENE = os.path.join(HERE, "golden", "scene16.npz")


def small_model(device):
    import fourier_feature_nets_amd as ffn
    g = np.load(os.path.join(HERE, "golden", "training.npz"))
    torch.manual_seed(0)
    model = ffn.PositionalFourierMLP(3, 4, 5.5, num_channels=64, embedding_size=48)
    sd = {k[len("fit_init/"):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("fit_init/")}
    model.load_state_dict(sd)
    return model.to(device)


def run_steps(group, steps, max_samples=None):
    """`steps` optimisation steps on ragged, non-stratified batches (so that the sharded and the
    unsharded run see the same samples) with annealing active.  Returns (losses, flat weights)."""
    import fourier_feature_nets_amd as ffn
    device = torch.device("cuda:0")
    model = small_model(device)
    with contextlib.redirect_stdout(io.StringIO()):
        train = ffn.ImageDataset.load(SCENE, "train", 16, True, False, anneal_start=0.2,
                                      num_anneal_steps=8, device=device)
    engine = ffn.TrainEngine(model, 0.0, group)
    if max_samples is not None:
        engine.max_samples = max_samples
    losses = []
    for step in range(steps):
        batch = torch.arange(step, len(train), 3, device=device)
        rays = train.ray_ids(batch)
        if rays.numel() % 2 == 0:          # odd on purpose: the two shards differ in size
            batch = batch[:-1]
        losses.append(float(engine.train_step(train, batch, step, 5e-4)))
    engine.check_finite()
    return losses, engine.flat.detach().cpu().clone()


def dp_train_worker(rank, world, port, out_path, steps, max_samples):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        losses, flat = run_steps(dist.group.WORLD, steps, max_samples)
        if rank == 0:
            torch.save({"losses": losses, "flat": flat}, out_path)
        dist.barrier()
    finally:
        dist.destroy_process_group()


def run_fit(group, steps=12, report=4):
    """`Raycaster.fit` for ``steps`` optimisation steps with a report (two validations, a log
    entry) every ``report`` steps, crop curriculum included, on a non-stratified training set so
    that sharded and unsharded runs see the same samples.  Epoch permutations come from ONE seed
    per epoch (np.random on rank 0).  Returns (printed lines, log psnrs, flat weights)."""
    import fourier_feature_nets_amd as ffn
    device = torch.device("cuda:0")
    np.random.seed(5)
    torch.manual_seed(5)
    model = small_model(device)
    with contextlib.redirect_stdout(io.StringIO()):
        train = ffn.ImageDataset.load(SCENE, "train", 16, True, False, anneal_start=0.2,
                                      num_anneal_steps=6, device=device)
        val = ffn.ImageDataset.load(SCENE, "val", 16, True, False, device=device)
    caster = ffn.Raycaster(model)
    caster.process_group = group
    caster.shuffle_source = "seeded"
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        log = caster.fit(train, val, 96, 5e-4, steps, 4, report, 0.1, 25000, 0.0, [])
    psnr = [(e.step, e.train_psnr, e.val_psnr) for e in log]
    return out.getvalue().splitlines(), psnr, caster.engine.flat.detach().cpu().clone()


def dp_fit_worker(rank, world, port, out_path):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        lines, psnr, flat = run_fit(dist.group.WORLD)
        torch.save({"lines": lines, "psnr": psnr, "flat": flat}, out_path + ".%d" % rank)
        dist.barrier()
    finally:
        dist.destroy_process_group()


# ------------------------------------------------------------------------------- scenarios
# Sharded steps held to a one-process run EXACTLY (tests/test_data_parallel_gpu.py).  A process
# without a group whose `max_samples` is one shard's sample count runs the shards of `world` ranks
# as its launches: same rays, same 1 / (3 * global count) scales, the same partial-sum loss path,
# and `grads.add_(part)` where two ranks' all-reduce computes g0 + g1.  One f32 addition is
# commutative, so the two runs must agree bit for bit -- while every rank does ONE launch per step
# and the reference's launches are the shards.  A third rank may join only with an empty shard (its
# reduce buffer is exactly zero, so the order of the sum does not matter).
# `prefetch`: whether `_can_prefetch` must allow the next step's samples to be drawn ahead (a rank
# then stores a look-ahead whenever its shard of the announced batch is not empty)
STEPS = 3
LEARNING_RATE = 5e-4
NOISE_SEED = 20240607

SCENARIOS = {
    # BASELINE config 4's combination: view directions, stratified jitter, focus samples from a
    # per-ray CDF table -- whose sampling may be drawn ahead of the optimiser update
    "nerf-table": dict(world=2, model="nerf", focus="table", stratified=True, prefetch=True),
    # the same with the coarse pass run per batch: nothing may be drawn ahead
    "nerf-live": dict(world=2, model="nerf", focus="live", stratified=True, prefetch=False),
    "nerf-bf16x6": dict(world=2, model="nerf", focus="table", stratified=True, prefetch=True,
                        precision="bf16x6"),
    # BASELINE config 5's: 512-wide Gaussian features, every rank compacting its own count
    "wide-occupancy": dict(world=2, model="wide", focus=None, stratified=False, prefetch=False,
                           occupancy=True),
    # 4, 1 and 3 valid rays over three ranks: shards (2,2,0), (1,0,0) and (1,1,1).  The step with
    # three contributions comes LAST: it is compared at a tolerance, and the weights it leaves
    # could not start another exact step
    "empty-shard": dict(world=3, model="small", focus=None, stratified=True, prefetch=True,
                        counts=(4, 1, 3)),
    # a batch with no valid ray between two ordinary ones
    "no-rays": dict(world=2, model="small", focus=None, stratified=True, prefetch=True,
                    counts=(None, 0, None)),
}


def shard_bounds(n, world):
    """[lo, hi) of every rank's slice of `n` rays: `TrainEngine.shard` restated
    (per = ceil(n / world), rays[rank * per:(rank + 1) * per])."""
    per = -(-n // world)
    return [(min(rank * per, n), min((rank + 1) * per, n)) for rank in range(world)]


def reference_max_samples(n, world, num_samples):
    """`max_samples` at which ONE process launches exactly the shards of `world` ranks."""
    return -(-n // world) * num_samples


def launch_bounds(count, max_samples, num_samples):
    """[lo, hi) of the launches `train_step` splits `count` rays into: its loop restated."""
    per_launch = max(1, max_samples // num_samples)
    return [(lo, min(lo + per_launch, count)) for lo in range(0, count, per_launch)]


def noise_widths(num_samples, stratified, focus):
    """Column counts of the `_noise` draws behind one sampling call, in draw order."""
    if not stratified:
        return ()
    if focus:
        return (num_samples // 2, num_samples - num_samples // 2)
    return (num_samples,)


def cut_noise(block, bounds, widths):
    """The pieces of one step's (global count, columns) noise block in the order a process draws
    them: per non-empty [lo, hi) of `bounds` its rows, cut into column groups of `widths`."""
    assert block.shape[1] == sum(widths)
    pieces = []
    for lo, hi in bounds:
        if hi <= lo:
            continue
        col = 0
        for width in widths:
            pieces.append(block[lo:hi, col:col + width])
            col += width
    return pieces


class NoiseFeed:
    """Stands in for `RaySampler._noise`: hands out prepared pieces in order.  A draw that was not
    planned, or one of another shape, fails there and then instead of shifting the stream."""

    def __init__(self, device):
        self.device = device
        self.pieces = []
        self.calls = 0

    def push(self, pieces):
        self.pieces.extend(p.contiguous().to(self.device) for p in pieces)

    def __call__(self, rows, count):
        self.calls += 1
        assert self.pieces, "unplanned noise draw (%d, %d)" % (rows, count)
        piece = self.pieces.pop(0)
        assert tuple(piece.shape) == (rows, count), (tuple(piece.shape), rows, count)
        return piece


_FIXTURES = {}


def _nerf_model(device):
    import fourier_feature_nets_amd as ffn
    from tests.golden.make_fit_schedule_nerf import NERF
    g = np.load(os.path.join(HERE, "golden", "fit_schedule_nerf.npz"))
    model = ffn.NeRF(**NERF)
    model.load_state_dict({k[len("init/"):]: torch.from_numpy(g[k]) for k in g.files
                           if k.startswith("init/")})
    return model.to(device)


def nerf_datasets(scene, focus_mode, device, stratified=True, with_val=False):
    """Training (and validation) set of the config-3 fixture (tests/test_round5_gpu.py::
    _replay_nerf_fit): the rig `tests.psnr_ensemble.write_npz` wrote to `scene`, focus samples
    guided by the `Voxels` opacity model of fit_schedule_nerf.npz."""
    import fourier_feature_nets_amd as ffn
    from tests.golden.make_fit_schedule_nerf import (ANNEAL_START, ANNEAL_STEPS, BATCH, SAMPLES,
                                                      VOXEL_SCALE, VOXEL_SIDE)
    g = np.load(os.path.join(HERE, "golden", "fit_schedule_nerf.npz"))
    opacity = ffn.Voxels(VOXEL_SIDE, VOXEL_SCALE)
    opacity.load_state_dict({"voxels": torch.from_numpy(g["opacity/voxels"]),
                             "bias": torch.from_numpy(g["opacity/bias"])})
    opacity = opacity.to(device)
    with contextlib.redirect_stdout(io.StringIO()):
        train = ffn.ImageDataset.load(scene, "train", SAMPLES, True, stratified, opacity, BATCH, "RGB",
                                      anneal_start=ANNEAL_START, num_anneal_steps=ANNEAL_STEPS,
                                      device=device, focus_mode=focus_mode)
        val = None
        if with_val:
            val = ffn.ImageDataset.load(scene, "val", SAMPLES, True, False, opacity, BATCH, "RGB",
                                        device=device, focus_mode=focus_mode)
    return train, val


def _scenario_dataset(spec, scene, device):
    """The scenario's training set, built once per process (`run_scenario` restores what it
    changes on it)."""
    import fourier_feature_nets_amd as ffn
    key = (spec["model"] == "nerf", spec["focus"], spec["stratified"])
    if key not in _FIXTURES:
        if spec["model"] == "nerf":
            assert scene is not None, "the NeRF scenarios need the rig file"
            _FIXTURES[key] = nerf_datasets(scene, spec["focus"], device, spec["stratified"])[0]
        else:
            with contextlib.redirect_stdout(io.StringIO()):
                _FIXTURES[key] = ffn.ImageDataset.load(SCENE, "train", 16, True, spec["stratified"],
                                                       anneal_start=0.2, num_anneal_steps=8, device=device)
    return _FIXTURES[key]


def _scenario_model(spec, device):
    if spec["model"] == "nerf":
        return _nerf_model(device)
    if spec["model"] == "wide":
        from tests import model_loaders
        return model_loaders.load_fourier(np.load(os.path.join(HERE, "golden", "models.npz")),
                                          "gaussian512", device)[0]
    return small_model(device)


def _own_occupancy(model, train, device, resolution=16):
    """A grid from the model's own density logits at the cell centres that keeps the cells above
    the MEDIAN density: part of the volume whatever the weights are, and the same bits in every
    process that holds the same weights."""
    import fourier_feature_nets_amd as ffn
    bounds = train.sampler.bounds
    centres = ffn.OccupancyGrid.cell_centres(bounds, resolution, device)
    model.eval()
    with torch.no_grad():
        logits = model(centres).contiguous()
    model.train()
    threshold = float(torch.nn.functional.softplus(logits[:, 3]).median())
    return ffn.OccupancyGrid.from_logits(logits, bounds, resolution, threshold, False)


def _scenario_rays(spec, train, device):
    """The filtered global ray ids of every step."""
    counts = spec.get("counts", (None,) * STEPS)
    every = train.ray_ids(torch.arange(0, len(train), 7, device=device))
    rays = []
    for step, count in enumerate(counts):
        if count is None:
            # the ragged every-third-ray batches of `run_steps`, odd so that the shards differ
            ids = train.ray_ids(torch.arange(step, len(train), 3, device=device))
            if ids.numel() % 2 == 0:
                ids = ids[:-1]
        else:
            ids = every[41 * step:41 * step + count]
            assert ids.numel() == count
        rays.append(ids.contiguous())
    return rays


def run_scenario(name, group, world, scene=None, shift=0, drop_second=False):
    """STEPS optimisation steps of scenario `name`: by this rank of `group`, or -- `group=None` --
    by one process that emulates `world` ranks with launches cut at the shard boundaries.

    `shift` / `drop_second` spoil the emulation on purpose (the controls): launches cut `shift`
    rays off the shard boundary, or only the first shard run at the full batch's scales.

    Returns a dict: `steps` (per step: loss, flat weights, both moments, grad_norm, the engine's
    step count, noise draws, whether a look-ahead is stored, evaluated fraction and compacted
    sample counts where a grid is set), `chunks` (every sampling call: the step it ran in, the step
    it sampled for, the ray ids), `moved` (largest weight change), `can_prefetch`; or
    {"refused": True} where the scenario's arithmetic mode has no kernels for the model and the
    step refuses it."""
    import fourier_feature_nets_amd as ffn
    spec = SCENARIOS[name]
    device = torch.device("cuda:0")
    rank = 0
    if group is not None:
        import torch.distributed as dist
        rank = dist.get_rank(group)
        assert dist.get_world_size(group) == world == spec["world"]
    train = _scenario_dataset(spec, scene, device)
    sampler = train.sampler
    num_samples = sampler.num_samples
    model = _scenario_model(spec, device)
    if "precision" in spec:
        model.train_precision = spec["precision"]
    rays = _scenario_rays(spec, train, device)
    engine = ffn.TrainEngine(model, 0.0, group)
    if "precision" in spec and not model.program().covers(spec["precision"]):
        # (every rank refuses before its collective: nobody is left waiting)
        try:
            engine.train_step(train, rays[0], 0, LEARNING_RATE, rays=rays[0])
        except NotImplementedError:
            return {"refused": True}
        raise AssertionError("a step in %s, which has no kernels for this model, was not refused"
                             % spec["precision"])
    grid_counts = []
    if spec.get("occupancy"):
        engine.occupancy = grid = _own_occupancy(model, train, device)
        compact = grid.compact

        def counting_compact(positions, views):
            out = compact(positions, views)
            grid_counts.append((int(positions.shape[0]), int(out[0].shape[0])))
            return out

        grid.compact = counting_compact
    widths = noise_widths(num_samples, spec["stratified"], spec["focus"])
    feed = NoiseFeed(device)
    planned = []          # per step: the [lo, hi) this process launches
    for step, ids in enumerate(rays):
        n = int(ids.numel())
        shards = shard_bounds(n, world)
        if group is not None:
            mine = [shards[rank]]
        elif drop_second:
            mine = [shards[0]]
        else:
            mine = launch_bounds(n, reference_max_samples(n, world, num_samples) + shift * num_samples,
                                 num_samples)
        planned.append([b for b in mine if b[1] > b[0]])
        if widths:
            block = torch.rand((n, sum(widths)), generator=torch.Generator().manual_seed(NOISE_SEED + step))
            feed.push(cut_noise(block, mine, widths))
    chunks, current = [], [None]
    orig_samples = ffn.TrainEngine._samples

    def recording_samples(self, smp, chunk, step):
        if self is engine:
            chunks.append({"during": current[0], "step": step, "rays": chunk.detach().cpu().clone()})
        return orig_samples(self, smp, chunk, step)

    start = engine.flat.detach().clone()
    steps = []
    sampler._noise = feed
    ffn.TrainEngine._samples = recording_samples
    try:
        for step, ids in enumerate(rays):
            n = int(ids.numel())
            current[0] = step
            if group is None:
                engine.max_samples = reference_max_samples(n, world, num_samples) + shift * num_samples
                if drop_second:
                    lo, hi = shard_bounds(n, world)[0]
                    engine.shard = lambda r, lo=lo, hi=hi: r[lo:hi].contiguous()
            ahead = None
            if group is not None and step + 1 < len(rays):
                # announced to EVERY scenario's ranks: where `_can_prefetch` is False it must be refused
                ahead = (train, rays[step + 1], step + 1)
            calls = feed.calls
            loss = engine.train_step(train, ids, step, LEARNING_RATE, rays=ids, lookahead=ahead)
            fraction = engine.last_evaluated_fraction
            steps.append({"loss": loss.detach().reshape(()).cpu().clone(),
                          "flat": engine.flat.detach().cpu().clone(),
                          "exp_avg": engine.exp_avg.detach().cpu().clone(),
                          "exp_avg_sq": engine.exp_avg_sq.detach().cpu().clone(),
                          "grad_norm": engine.grad_norm.detach().cpu().clone(),
                          "count": engine.count,
                          "noise_calls": feed.calls - calls,
                          "prefetched": getattr(engine, "_prefetched", None) is not None,
                          "fraction": None if fraction is None else float(fraction),
                          "compacted": list(grid_counts)})
            del grid_counts[:]
        engine.check_finite()
    finally:
        ffn.TrainEngine._samples = orig_samples
        del sampler._noise            # (the instance attribute: the class's method is back)
    assert not feed.pieces, "%d planned noise pieces were never drawn" % len(feed.pieces)
    return {"steps": steps, "chunks": chunks, "planned": planned, "noise_widths": widths,
            "moved": float((engine.flat - start).abs().max()),
            "can_prefetch": bool(engine._can_prefetch(sampler)),
            "counts": [int(ids.numel()) for ids in rays]}


def dp_scenarios_worker(rank, world, port, out_dir, names, scene):
    """One rank of `world` (gloo, sharing cuda:0) through every scenario of `names`."""
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        for name in names:
            torch.save(run_scenario(name, dist.group.WORLD, world, scene),
                       os.path.join(out_dir, "%s.%d.pt" % (name, rank)))
        dist.barrier()
    finally:
        dist.destroy_process_group()
