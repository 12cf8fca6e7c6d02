"""Voxel radiance-field training on the GPU: the K10b backward (csrc/voxels.hip) against ATen's
grid_sample backward in float64, its adjoint identity with K10, its determinism and argument
refusals; `Voxels` through `TrainEngine` / `Raycaster.fit` replayed against the reference's own
`fit` (tests/golden/fit_schedule_voxels.npz); the K10 forward against grid_sample in float64
(``check_forward``); and the README workflow train_voxels.py -> --opacity-model end to end.

Error budgets follow tests/composite_reference.py: every element is held to
kappa * 2^-24 * budget, the budget being a first-order f32 error bound of that element:

    summation   (M + 4) * sum_i |g_i| w_i   M = contributions of the voxel (samples in its 8 cells),
                                             +4 for the rounding of the weight product itself
    coordinates 12 (S + 1) * sum_i |g_i|     the f32 voxel coordinate ((p/scale + 1) S - 1) / 2 is
                                             within 4 (S + 1) ulp(1) of the exact one; a weight moves
                                             by at most that much per axis, three axes
"""

import contextlib
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SCENE = os.path.join(GOLDEN, "scene16.npz")
U = 2.0 ** -24
KAPPA = 1.0


def dev():
    return torch.device("cuda:0")


def _quiet(fn, *args, **kwargs):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*args, **kwargs)


# ----------------------------------------------------------------------------------- float64 reference
def _grid_backward64(pos, g, side, scale):
    """ATen's grid_sample backward (border, align_corners=False) in float64 on the CPU:
    d(sum_i g_i . grid_sample(vol)(p_i / scale)) / d vol -> (4,S,S,S)."""
    vol = torch.zeros((1, 4, side, side, side), dtype=torch.float64, requires_grad=True)
    grid = (pos.double().cpu() / scale).reshape(1, -1, 1, 1, 3)
    out = F.grid_sample(vol, grid, padding_mode="border", align_corners=False)    # (1,4,N,1,1)
    out.backward(g.double().cpu().t().reshape(1, 4, -1, 1, 1))
    return vol.grad[0]


def _cells64(pos, side, scale):
    c = ((pos.double().cpu() / scale + 1) * side - 1) / 2
    c = c.clamp(0, side - 1)
    lo = c.floor().long()
    return (lo[:, 2] * side + lo[:, 1]) * side + lo[:, 0]


def _corner_sum(per_cell, side):
    """per-voxel sum over the (up to) 8 cells the voxel is a corner of."""
    grid = per_cell.reshape(-1, side, side, side)
    out = grid.clone()
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                if dx == dy == dz == 0:
                    continue
                out[:, dz:, dy:, dx:] += grid[:, :side - dz, :side - dy, :side - dx]
    return out


def backward_budget(pos, g, side, scale, coordinates=True):
    """(reference (4,S,S,S), budget (4,S,S,S)) in float64; ``coordinates=False``: the summation
    part only (kernels that share K10's f32 weights)."""
    ref = _grid_backward64(pos, g, side, scale)
    absw = _grid_backward64(pos, g.abs(), side, scale)
    cells = _cells64(pos, side, scale)
    count = torch.zeros((side ** 3,), dtype=torch.float64).index_add_(0, cells, torch.ones_like(cells, dtype=torch.float64))
    gabs = torch.zeros((4, side ** 3), dtype=torch.float64).index_add_(1, cells, g.double().cpu().abs().t())
    m = _corner_sum(count.reshape(1, -1), side)
    b = _corner_sum(gabs, side)
    return ref, (m + 4) * absw + (12 * (side + 1) * b if coordinates else 0)


def check_backward(pos, g, side, scale, label=""):
    from fourier_feature_nets_amd import ops
    d_vol = torch.full((4, side, side, side), float("nan"), device=dev())
    d_bias = torch.full((4,), float("nan"), device=dev())
    ops.voxels_backward(pos, g, side, scale, d_volume=d_vol, d_bias=d_bias)
    got = d_vol.double().cpu()
    assert torch.isfinite(got).all(), label
    ref, budget = backward_budget(pos, g, side, scale)
    err = (got - ref).abs()
    ratio = float((err / (KAPPA * U * budget + 1e-300)).max())
    assert (err <= KAPPA * U * budget).all(), (label, ratio)
    gb = g.double().cpu()
    bias_ref = gb.sum(0)
    bias_budget = len(gb) * gb.abs().sum(0)
    assert ((d_bias.double().cpu() - bias_ref).abs() <= U * bias_budget).all(), label
    return d_vol, d_bias, ratio


def _positions(n, side, scale, seed, spread=1.3):
    """Uniform in a cube a bit larger than the volume, plus points exactly on the faces, on the
    S-1 clamp, on voxel centres and at the cube's corners."""
    gen = torch.Generator().manual_seed(seed)
    pos = (torch.rand((n, 3), generator=gen) * 2 - 1) * spread * scale
    special = []
    for axis in range(3):
        for v in (-1.0, 1.0, -1.0 + 1.0 / side, 1.0 - 1.0 / side, 0.0):   # faces, outermost centres, middle
            p = (torch.rand((16, 3), generator=gen) * 2 - 1) * scale
            p[:, axis] = v * scale
            special.append(p)
    corners = torch.tensor([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)],
                           dtype=torch.float32) * scale
    special.append(corners)
    special.append(corners * 3)              # outside: clamped to the border
    return torch.cat([pos] + special).float().contiguous()


@pytest.mark.parametrize("side,scale", [(1, 1.0), (5, 1.5), (8, 1.0), (32, 0.7), (128, 1.0)])
def test_backward_against_grid_sample_float64(side, scale):
    """K10b against ATen's grid_sample backward in float64 from the same f32 positions, every
    entry within its budget (see the module docstring); d_bias = the column sums of d_logits
    within n * sum|g| * 2^-24.  Positions include points outside the cube, exactly on its faces,
    on the S-1 clamp and at its corners; every output starts as NaN."""
    n = 20000 if side < 128 else 200000
    pos = _positions(n, side, scale, seed=side)
    g = torch.randn((pos.shape[0], 4), generator=torch.Generator().manual_seed(3 + side))
    _, _, ratio = check_backward(pos.to(dev()), g.to(dev()).contiguous(), side, scale, "S=%d" % side)
    print("S=%d worst error / budget %.3g" % (side, ratio))


def _heavy(n=120000, side=32):
    """>= 1e5 samples in <= 4 cells (long lists: the chunked path), plus a scattered background."""
    gen = torch.Generator().manual_seed(5)
    centres = torch.tensor([[0.1, 0.2, -0.3], [0.11, 0.2, -0.3], [-0.5, 0.5, 0.5], [0.9, -0.9, 0.0]])
    cell = 2.0 / side
    which = torch.randint(0, 4, (n,), generator=gen)
    # a cell of the lookup spans two neighbouring voxel centres (k + 1/2) * cell - 1
    first = ((centres + 1) / cell - 0.5).floor() * cell - 1 + cell * 0.5
    pos = first[which] + (0.05 + 0.9 * torch.rand((n, 3), generator=gen)) * cell
    back = (torch.rand((5000, 3), generator=gen) * 2 - 1)
    pos = torch.cat([pos, back]).contiguous()
    g = torch.randn((pos.shape[0], 4), generator=gen)
    return pos, g


def test_backward_heavy_collision_budget_and_bits():
    """>= 1e5 samples in 4 cells: within budget, and 10 calls give bit-identical d_volume / d_bias
    (no float atomics on any path)."""
    from fourier_feature_nets_amd import ops
    side, scale = 32, 1.0
    pos, g = _heavy(side=side)
    cells = _cells64(pos, side, scale)
    assert int(torch.bincount(cells).topk(4).values.sum()) >= 100000
    pos, g = pos.to(dev()), g.to(dev())
    d_vol, d_bias, ratio = check_backward(pos, g, side, scale, "heavy")
    print("heavy worst error / budget %.3g" % ratio)
    ws = torch.empty(((ops.voxels_backward_workspace_bytes(pos.shape[0], side) + 3) // 4,), device=dev())
    for _ in range(10):
        v2, b2 = ops.voxels_backward(pos, g, side, scale, workspace=ws)
        assert torch.equal(v2.view(torch.int32), d_vol.view(torch.int32))
        assert torch.equal(b2.view(torch.int32), d_bias.view(torch.int32))


@pytest.mark.parametrize("side,scale", [(5, 1.5), (32, 0.7)])
def test_adjoint_identity_with_k10(side, scale):
    """<K10(v) - bias, g> = <v, K10b(g)> in float64 (an axis or layout mistake breaks it by O(1)):
    both sides are computed from the kernels' f32 outputs; the gap is bounded by the forward's
    8-term sums (16 u per sample) and the backward's summation budget (both use the same f32
    weights, so no coordinate term)."""
    from fourier_feature_nets_amd import ops
    pos = _positions(30000, side, scale, seed=11).to(dev())
    gen = torch.Generator().manual_seed(12)
    vol = torch.randn((4, side, side, side), generator=gen).to(dev())
    bias = torch.randn((4,), generator=gen).to(dev())
    g = torch.randn((pos.shape[0], 4), generator=gen).to(dev())
    fwd = ops.voxels_forward(vol, bias, pos, side, scale)
    lhs = float(((fwd.double() - bias.double()) * g.double()).sum())
    d_vol, _ = ops.voxels_backward(pos, g, side, scale)
    rhs = float((vol.double() * d_vol.double()).sum())
    fabs = ops.voxels_forward(vol.abs(), torch.zeros_like(bias), pos, side, scale).double()
    _, budget = backward_budget(pos, g, side, scale, coordinates=False)
    bound = U * (16 * float((fabs * g.double().abs()).sum())
                 + float((vol.double().abs().cpu() * budget).sum()))
    assert abs(lhs - rhs) <= bound, (lhs, rhs, bound)
    # the same identity with one axis of the backward transposed fails by far
    wrong = float((vol.double() * d_vol.double().transpose(1, 3)).sum())
    assert abs(lhs - wrong) > 10 * bound


def test_refusals_launch_nothing():
    """Bad side, n or scale -> FfnError before any launch: the outputs keep their sentinel."""
    import fourier_feature_nets_amd as ffn
    from fourier_feature_nets_amd import _lib, ops
    pos = torch.zeros((8, 3), device=dev())
    g = torch.ones((8, 4), device=dev())
    for side, scale in [(0, 1.0), (1025, 1.0), (-3, 1.0), (4, 0.0), (4, -1.0), (4, float("nan")),
                        (4, float("inf"))]:
        d_vol = torch.full((4 * max(side, 1) ** 3 if 0 < side <= 64 else 4,), 7.0, device=dev())
        d_bias = torch.full((4,), 7.0, device=dev())
        ws = torch.zeros((1 << 16,), device=dev())
        with pytest.raises(_lib.FfnError):
            ops._call("ffn_voxels_backward", ops._dev(pos), ops._dev(g), _lib.c_i64(8), _lib.c_i(side),
                      _lib.c_f(scale), ops._dev(ws), _lib.c_i64(ws.numel() * 4), ops._dev(d_vol),
                      ops._dev(d_bias))
        torch.cuda.synchronize()
        assert bool((d_vol == 7.0).all()) and bool((d_bias == 7.0).all()), (side, scale)
    d_vol = torch.full((4 * 4 ** 3,), 7.0, device=dev())
    d_bias = torch.full((4,), 7.0, device=dev())
    ws = torch.zeros((1 << 16,), device=dev())
    for n, ws_bytes in [(-1, ws.numel() * 4), ((1 << 30) + 1, ws.numel() * 4), (8, 64)]:
        with pytest.raises(_lib.FfnError):
            ops._call("ffn_voxels_backward", ops._dev(pos), ops._dev(g), _lib.c_i64(n), _lib.c_i(4),
                      _lib.c_f(1.0), ops._dev(ws), _lib.c_i64(ws_bytes), ops._dev(d_vol), ops._dev(d_bias))
    torch.cuda.synchronize()
    assert bool((d_vol == 7.0).all()) and bool((d_bias == 7.0).all())
    with pytest.raises(ffn.ops._lib.FfnError):
        ops.voxels_backward_workspace_bytes(8, 0)
    # n = 0 still writes every entry
    d_vol, d_bias = ops.voxels_backward(pos[:0], g[:0], 4, 1.0)
    assert not bool(d_vol.any()) and not bool(d_bias.any())


# ----------------------------------------------------------------------------------- training steps
def _voxel_engine(side=16, **kw):
    import fourier_feature_nets_amd as ffn
    torch.manual_seed(4)
    model = ffn.Voxels(side, 1.0)
    with torch.no_grad():
        model.voxels.normal_(0, 0.5)
    return ffn.TrainEngine(model.to(dev()), **kw), model


def _dataset(stratified):
    import fourier_feature_nets_amd as ffn
    ds = _quiet(ffn.ImageDataset.load, SCENE, "train", 32, True, stratified, device=dev())
    ds.sampler.noise_source = "host"
    return ds


def test_voxel_train_steps_are_bit_identical():
    """Two voxel train_steps from the same state and noise give bit-identical flat parameters,
    Adam moments and losses; the program has 4 S^3 + 4 gradient floats; Voxels gains no
    `program` attribute."""
    ds = _dataset(True)
    batch = torch.arange(0, len(ds), 3, device=dev())
    runs = []
    for _ in range(2):
        engine, model = _voxel_engine()
        torch.manual_seed(9)
        loss = engine.train_step(ds, batch, 0, 0.01)
        torch.manual_seed(10)
        loss2 = engine.train_step(ds, batch, 1, 0.01)
        runs.append((engine.flat.clone(), engine.exp_avg_sq.clone(), float(loss), float(loss2)))
        assert engine.flat.numel() == 4 * 16 ** 3 + 4
        assert not hasattr(model, "program")
    (f0, v0, a0, b0), (f1, v1, a1, b1) = runs
    assert torch.equal(f0.view(torch.int32), f1.view(torch.int32))
    assert torch.equal(v0.view(torch.int32), v1.view(torch.int32))
    assert (a0, b0) == (a1, b1)
    assert not torch.equal(f0, _voxel_engine()[0].flat)          # the step did move the volume


def test_voxel_step_split_into_launches_matches_one_launch(monkeypatch):
    """max_samples_per_launch small (several forward/backward launches whose gradients are summed)
    gives the one-launch gradient within the f32 budget of the two summation orders."""
    import fourier_feature_nets_amd as ffn
    ds = _dataset(False)
    batch = torch.arange(0, len(ds), 2, device=dev())
    seen, grads = [], []
    real_bwd, real_adam = ffn.VoxelProgram.backward, ffn.ops.clip_adam

    def bwd(self, d_logits, positions, views, saved, g, precision="f32"):
        seen.append((positions.clone(), d_logits.clone()))
        return real_bwd(self, d_logits, positions, views, saved, g, precision)

    def adam(params, g, *a, **k):
        grads.append(g.clone())
        return real_adam(params, g, *a, **k)

    monkeypatch.setattr(ffn.VoxelProgram, "backward", bwd)
    monkeypatch.setattr(ffn.ops, "clip_adam", adam)
    engine, _ = _voxel_engine()
    engine.train_step(ds, batch, 0, 0.01)
    one = seen[:]
    seen.clear()
    engine2, _ = _voxel_engine(max_samples_per_launch=32 * 40)
    engine2.train_step(ds, batch, 0, 0.01)
    assert len(one) == 1 and len(seen) > 3
    side = 16
    pos = torch.cat([p for p, _ in seen])
    g = torch.cat([d for _, d in seen])
    assert torch.equal(pos, one[0][0])
    _, budget = backward_budget(pos, g, side, 1.0)
    cut = 4 * side ** 3
    err = (grads[0][:cut] - grads[1][:cut]).double().abs().cpu().reshape(4, side, side, side)
    assert (err <= 2 * U * budget + 1e-30).all()
    gb = g.double().abs().sum(0).cpu()
    assert ((grads[0][cut:] - grads[1][cut:]).double().abs().cpu() <= 2 * U * len(g) * gb).all()


def test_occupancy_schedule_with_voxels_raises():
    import fourier_feature_nets_amd as ffn
    ds = _dataset(True)
    caster = ffn.Raycaster(ffn.Voxels(8, 1.0).to(dev()))
    caster.train_occupancy_schedule = (0, 1)
    with pytest.raises(NotImplementedError):
        caster.fit(ds, ds, 64, 0.01, 1, 0, 1, 0.9, 25000, 0.0, [])
    engine, _ = _voxel_engine()
    engine.occupancy = object()
    with pytest.raises(NotImplementedError):
        engine.train_step(ds, torch.arange(0, 64, device=dev()), 0, 0.01)


# ----------------------------------------------------------------------------------- K10 forward
# K10's forward against float64: element budget (units of 2^-24) per output channel
#     summation    12 (sum_k |v_k w_k| + |bias|)     weights 1 - f and two products, eight products,
#                                                   seven additions, the bias
#     coordinates  sum_d D_d delta_d                delta_d: the f32 coordinate's error bound
#                                                   (1/scale rounded on the host, the kernel's
#                                                   fma((p, inv, 1)) * S - 1), D_d: the largest corner
#                                                   difference along axis d over the cell and its
#                                                   neighbours (the f32 coordinate may sit in the next
#                                                   cell where the exact one lies within delta_d of an
#                                                   integer)
KAPPA_FORWARD = 0.4      # about twice the worst ratio measured on an MI355X over the cases below [0.201, S=2]
FORWARD_TEETH = ("align_corners", "zeros_padding", "xz_swapped", "no_bias")


def _forward64(vol, bias, pos, scale, variant=None):
    """grid_sample of p / scale (border, align_corners=False) + bias in float64 on vol's device; (N,4)."""
    grid = pos.double() / scale
    if variant == "xz_swapped":
        grid = grid[:, [2, 1, 0]]
    out = F.grid_sample(vol.double()[None], grid.reshape(1, -1, 1, 1, 3),
                        padding_mode="zeros" if variant == "zeros_padding" else "border",
                        align_corners=variant == "align_corners")
    out = out.reshape(4, -1).t()
    return out if variant == "no_bias" else out + bias.double()


def forward_budget(vol, bias, pos, side, scale):
    """(N,4) budget in units of 2^-24 of K10 at ``pos`` (see the block comment)."""
    v = vol.double()
    x = pos.double() / scale
    c = (((x + 1) * side - 1) / 2).clamp(0, side - 1)
    lo = c.floor().long().clamp(max=side - 1)
    f = c - lo
    hi = (lo + 1).clamp(max=side - 1)
    u = 2.0 ** -24
    # |c32 - c| / u: inv = 1/scale (1 + e), fma(p, inv, 1), * S, - 1, * 0.5 (exact)
    delta = (side * (x.abs() + (x + 1).abs()) + ((x + 1) * side).abs() + ((x + 1) * side - 1).abs()) / 2 + 1
    flat = lambda z, y, xx: (z * side + y) * side + xx            # noqa: E731
    vf = v.reshape(4, -1)
    sum_abs = torch.zeros((pos.shape[0], 4), dtype=torch.float64, device=pos.device)
    for cz in (0, 1):
        for cy in (0, 1):
            for cx in (0, 1):
                w = ((f[:, 0] if cx else 1 - f[:, 0]) * (f[:, 1] if cy else 1 - f[:, 1])
                     * (f[:, 2] if cz else 1 - f[:, 2]))
                idx = flat((hi if cz else lo)[:, 2], (hi if cy else lo)[:, 1], (hi if cx else lo)[:, 0])
                sum_abs += (vf[:, idx].t() * w[:, None]).abs()
    budget = 12 * (sum_abs + bias.double().abs())
    for d in range(3):                      # x is the last volume axis
        axis = 3 - d
        if side > 1:                        # |v[i + 1] - v[i]| along the axis, 0 at the last voxel
            diff = (v.narrow(axis, 1, side - 1) - v.narrow(axis, 0, side - 1)).abs()
            diff = F.pad(diff, [0, int(axis == 3), 0, int(axis == 2), 0, int(axis == 1)])
        else:
            diff = torch.zeros_like(v)
        near = F.max_pool3d(diff[None], 3, 1, 1)[0].reshape(4, -1)    # the cell's neighbours
        dmax = torch.zeros((pos.shape[0], 4), dtype=torch.float64, device=pos.device)
        for cz in (lo, hi):
            for cy in (lo, hi):
                for cx in (lo, hi):
                    dmax = torch.maximum(dmax, near[:, flat(cz[:, 2], cy[:, 1], cx[:, 0])].t())
        budget += dmax * delta[:, d:d + 1]
    return budget


def check_forward(vol, bias, pos, side, scale, label=""):
    """K10 from NaN-filled outputs against ``_forward64`` within KAPPA_FORWARD * 2^-24 * budget; the
    teeth (changed references) must each be failed somewhere.  Returns the worst ratio and the
    teeth's smallest multiples of the bound."""
    from fourier_feature_nets_amd import ops
    n = pos.shape[0]
    out = torch.full((n, 4), float("nan"), device=dev())
    ops._call("ffn_voxels_forward", ops._dev(vol), ops._dev(bias), ops._dev(pos, name="positions"),
              ops._lib.c_i64(n), ops._lib.c_i(side), ops._lib.c_f(scale), ops._dev(out))
    got = out.double()
    ref = _forward64(vol, bias, pos, scale)
    bound = KAPPA_FORWARD * U * forward_budget(vol, bias, pos, side, scale)
    err = (got - ref).abs()
    ratio = float((err / bound).max())
    assert bool(torch.isfinite(got).all()), label
    assert bool((err <= bound).all()), (label, ratio, int((err > bound).sum()))
    teeth = {}
    for name in FORWARD_TEETH:
        alt = _forward64(vol, bias, pos, scale, name)
        touched = (alt - ref).abs() > bound
        if bool(touched.any()):
            teeth[name] = float(((got - alt).abs() / bound)[touched].max())
    return ratio, teeth


@pytest.mark.parametrize("side,scale", [(1, 1.0), (2, 0.8), (5, 1.5), (8, 1.0), (32, 0.7), (128, 1.0),
                                        (256, 1.3)])
def test_forward_against_grid_sample_float64(side, scale):
    """K10 against float64 grid_sample + bias on _positions (faces, the S-1 clamp, voxel centres,
    corners, outside the cube); every tooth must touch the data and be failed."""
    gen = torch.Generator().manual_seed(side)
    vol = torch.randn((4, side, side, side), generator=gen).to(dev())
    bias = torch.randn((4,), generator=gen).to(dev())
    pos = _positions(20000, side, scale, seed=side + 1).to(dev())
    ratio, teeth = check_forward(vol, bias, pos, side, scale, "S=%d" % side)
    print("K10 forward S=%d worst error / budget %.3g, teeth %s" % (side, ratio, teeth))
    want = [t for t in FORWARD_TEETH if side > 1 or t in ("zeros_padding", "no_bias")]   # (S = 1: constant)
    for name in want:
        assert name in teeth and teeth[name] > 1.0, (name, teeth)


def test_forward_past_the_grid_stride_cap():
    """More samples than 8192 workgroups x 256 threads: every thread loops; all written."""
    side, scale = 8, 1.0
    gen = torch.Generator().manual_seed(3)
    vol = torch.randn((4, side, side, side), generator=gen).to(dev())
    bias = torch.randn((4,), generator=gen).to(dev())
    n = 8192 * 256 + 4099
    pos = ((torch.rand((n, 3), generator=gen) * 2 - 1) * 1.1).to(dev())
    ratio, teeth = check_forward(vol, bias, pos, side, scale, "cap")
    print("K10 forward cap worst error / budget %.3g, teeth %s" % (ratio, teeth))


# ----------------------------------------------------------------------------------- the reference's fit replayed
def test_fit_schedule_voxels_replays_the_reference(tmp_path):
    """`Raycaster.fit` on a Voxels(32, 2/bounds[0,0]) model replayed against the reference's own
    run (tests/golden/fit_schedule_voxels.npz from make_fit_schedule_voxels.py): 15 optimiser
    steps, lr 0.01, stratified with annealing, crop_steps 0, reports every 5.  Every training batch
    must equal the reference's EXACTLY.  Tolerances: the reference divides positions by the
    scale where K10 multiplies by its f32 reciprocal, and ATen sums the scatter in another order,
    so gradients differ in the last bits; Adam's first steps move each touched voxel by about
    lr * g / |g|, which keeps those relative differences relative (|g| >> eps for every voxel a
    sample touches).  Measured on an MI355X: losses 1.2e-7 relative, PSNR columns 6e-7 dB, final
    state 1.9e-6 absolute (the volume moves by up to 15 * lr = 0.15); held to about ten times
    that: losses 2e-6 relative, PSNR 1e-5 dB, state 2e-5."""
    import fourier_feature_nets_amd as ffn
    from tests.golden.make_fit_schedule_voxels import (ANNEAL_STEPS, BATCH, DECAY_RATE, DECAY_STEPS, LR,
                                                       NUM_STEPS, REPORT, SAMPLES, SIDE, SIZE, TRAIN_CAMS,
                                                       VAL_CAMS)
    from tests.psnr_ensemble import write_npz
    g = np.load(os.path.join(GOLDEN, "fit_schedule_voxels.npz"))
    npz = write_npz(str(tmp_path / "scene.npz"), TRAIN_CAMS, VAL_CAMS, SIZE)
    train = _quiet(ffn.ImageDataset.load, npz, "train", SAMPLES, True, True, anneal_start=0.2,
                   num_anneal_steps=ANNEAL_STEPS, device=dev())
    val = _quiet(ffn.ImageDataset.load, npz, "val", SAMPLES, True, False, device=dev())
    train.sampler.noise_source = "host"
    scale = 2 / float(train.sampler.bounds[0, 0])
    assert abs(scale - float(g["scale"])) < 1e-7
    model = ffn.Voxels(SIDE, scale)
    model.load_state_dict({k[len("init/"):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("init/")})
    model = model.to(dev())
    torch.manual_seed(777)
    np.random.seed(777)
    caster = ffn.Raycaster(model)
    batches = []
    orig_init, orig_step = ffn.TrainEngine.__init__, ffn.TrainEngine.train_step

    def recording_init(self, *a, **k):
        orig_init(self, *a, **k)
        self.loss_history = []

    def recording_step(self, dataset, batch, step, lr, rays=None, **kw):
        batches.append(torch.as_tensor(batch).cpu().numpy().astype(np.int64))
        return orig_step(self, dataset, batch, step, lr, rays=rays, **kw)

    ffn.TrainEngine.__init__, ffn.TrainEngine.train_step = recording_init, recording_step
    buf = io.StringIO()
    try:
        with contextlib.redirect_stdout(buf):
            log = caster.fit(train, val, BATCH, LR, NUM_STEPS, 0, REPORT, DECAY_RATE, DECAY_STEPS, 0.0, [])
    finally:
        ffn.TrainEngine.__init__, ffn.TrainEngine.train_step = orig_init, orig_step
    assert len(batches) == len(g["batches"]) == NUM_STEPS + 1
    for step, (mine, theirs) in enumerate(zip(batches, g["batches"])):
        assert np.array_equal(mine, theirs), step
    losses = np.array([float(x) for x in caster.engine.loss_history])
    state = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    worst = {"loss_rel": float(np.max(np.abs(losses / g["losses"] - 1))),
             "train_psnr": float(np.max(np.abs(np.array([e.train_psnr for e in log]) - g["log_train_psnr"]))),
             "val_psnr": float(np.max(np.abs(np.array([e.val_psnr for e in log]) - g["log_val_psnr"]))),
             "state": max(float(np.max(np.abs(state[k[6:]] - g[k]))) for k in g.files if k.startswith("final/"))}
    print("fit replay worst deviations", worst)
    assert list(state) == ["voxels", "bias"]
    assert [e.step for e in log] == g["log_steps"].tolist()
    np.testing.assert_allclose(losses, g["losses"], rtol=2e-6, atol=0)
    np.testing.assert_allclose([e.train_psnr for e in log], g["log_train_psnr"], rtol=0, atol=1e-5)
    np.testing.assert_allclose([e.val_psnr for e in log], g["log_val_psnr"], rtol=0, atol=1e-5)
    mine = [ln.split() for ln in buf.getvalue().splitlines() if ln[:7].isdigit()]
    theirs = [ln.split() for ln in str(g["stdout"]).splitlines() if ln[:7].isdigit()]
    assert len(mine) == len(theirs)
    for a, b in zip(mine, theirs):
        assert a[0] == b[0] and abs(float(a[4]) - float(b[4])) < 5e-3 and abs(float(a[6]) - float(b[6])) < 5e-3
    for key in g.files:
        if key.startswith("final/"):
            np.testing.assert_allclose(state[key[len("final/"):]], g[key], rtol=0, atol=2e-5)


# ----------------------------------------------------------------------------------- README workflow
def test_train_voxels_then_opacity_model_workflow(tmp_path):
    """README workflow: scripts/train_voxels.py on a synthetic scene writes voxels.pt + log.txt;
    load_model returns a Voxels with the reference's keys; train_nerf.py --opacity-model runs 2
    steps with the table and the live focus sampler."""
    import fourier_feature_nets_amd as ffn
    scene = str(tmp_path / "scene.npz")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "make_synthetic_npz.py"), scene,
                          "--size", "32", "--cameras", "12"], capture_output=True, text=True, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    out = str(tmp_path / "vox")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train_voxels.py"), scene, "16", out,
                          "--num-steps", "4", "--report-interval", "2", "--image-interval", "100",
                          "--batch-size", "128", "--num-samples", "32"],
                         capture_output=True, text=True, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    assert "voxels.pt" in os.listdir(out) and "log.txt" in os.listdir(out)
    with open(os.path.join(out, "log.txt")) as f:
        lines = f.read().strip().split("\n")
    assert [ln.split("\t")[0] for ln in lines[3:]] == ["0", "2", "4"]
    model = ffn.load_model(os.path.join(out, "voxels.pt"))
    assert isinstance(model, ffn.Voxels) and list(model.state_dict()) == ["voxels", "bias"]
    assert model.params["side"] == 16 and not bool((model.voxels == 0).all())
    blob = torch.load(os.path.join(out, "voxels.pt"), map_location="cpu")
    assert blob["type"] == "voxels" and set(blob) == {"voxels", "bias", "type", "params"}
    for mode in ("table", "live"):
        run = str(tmp_path / ("nerf_" + mode))
        res = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train_nerf.py"), scene, run,
                              "--opacity-model", os.path.join(out, "voxels.pt"), "--focus-mode", mode,
                              "--num-steps", "1", "--report-interval", "1", "--image-interval", "100",
                              "--batch-size", "64", "--num-samples", "16", "--num-layers", "3",
                              "--num-channels", "64", "--crop-steps", "0"],
                             capture_output=True, text=True, cwd=ROOT)
        assert res.returncode == 0, (mode, res.stderr[-2000:])
        assert "nerf.pt" in os.listdir(run)
