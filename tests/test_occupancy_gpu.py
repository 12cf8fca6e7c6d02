"""K9 occupancy kernels (csrc/occupancy.hip) at their exact edges.  Every answer is an integer or a
copied float, so every comparison is exact:

* build: G = 1, 5, 33, 64 (125 and 35 937 cells end inside a 32-bit word; the bits past G^3 must be 0)
  against a float64 softplus and the strict ``> threshold``; on the ``x > 20`` identity branch the
  kernel's value is x itself, so the decision is exact there, elsewhere either answer is accepted
  within a few ulps of the threshold;
* dilation: ``max_pool3d`` of the kernel's own undilated bits;
* count / scan / compact: ``_cpu_occupied`` (NaN positions occupied) at n = 1, 262 144 +- 1 and about
  3e6 (above 1024 blocks a thread of the one-workgroup scan takes more than one block count), with
  positions on cell boundaries and box faces, with and without views;
* scatter / gather at m = 0 and m = n, the gather being the scatter's inverse.
Outputs start filled with a sentinel, so an unwritten word fails."""

import math
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fourier_feature_nets_amd import ops
from fourier_feature_nets_amd._lib import c_f, c_i, c_i64
from tests.test_round2_gpu import _cpu_occupied

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def dev():
    return torch.device("cuda:0")


def _build(logits, G, threshold, dilate):
    """ffn_occupancy_build with the output (and the scratch) pre-filled with all ones."""
    words = (G ** 3 + 31) // 32
    bits = torch.full((words,), -1, dtype=torch.int32, device=dev())
    scratch = torch.full((words,), -1, dtype=torch.int32, device=dev()) if dilate else None
    ops._call("ffn_occupancy_build", ops._dev(logits), c_i(G), c_f(threshold), c_i(1 if dilate else 0),
              ops._dev(scratch, torch.int32), ops._dev(bits, torch.int32))
    torch.cuda.synchronize()
    return bits.cpu()


def _unpack(bits):
    words = bits.to(torch.int64) & 0xffffffff
    return ((words[:, None] >> torch.arange(32)) & 1).reshape(-1).bool()


def _logits(G, threshold, seed):
    """(G^3, 4) float32: sigma logits spread over both softplus branches, some exactly at 20, some
    whose softplus lands on the threshold, and (for thresholds above 20) some equal to it."""
    gen = torch.Generator().manual_seed(seed)
    n = G ** 3
    x = torch.randn(n, generator=gen, dtype=torch.float64) * 3 + math.log(math.expm1(threshold))
    x = x.float()
    k = torch.randint(0, 6, (n,), generator=gen)
    on = float(np.float32(math.log(math.expm1(threshold))))
    x = torch.where(k == 1, torch.tensor(on), x)
    x = torch.where(k == 2, torch.tensor(20.0), x)
    x = torch.where(k == 3, torch.tensor(float(np.nextafter(np.float32(20), np.float32(30)))), x)
    x = torch.where(k == 4, torch.tensor(float(np.float32(threshold))), x)
    out = torch.randn((n, 4), generator=gen)
    out[:, 3] = x
    return out


def _build_expected(x, threshold):
    """(decided, value): the float64 decision of softplus(x) > threshold, and where it is decided."""
    t = float(np.float32(threshold))
    xd = x.double()
    ident = x > 20.0
    sp = torch.where(ident, xd, torch.log1p(torch.exp(xd)))
    want = sp > t
    decided = ident | ((sp - t).abs() > 8 * U * max(abs(t), 1e-30) + 2.0 ** -140)
    return decided, want


@pytest.mark.parametrize("G", [1, 5, 33, 64])
@pytest.mark.parametrize("threshold", [0.5, 20.0, 20.5])
def test_build_and_dilate_exact(G, threshold):
    logits = _logits(G, threshold, G)
    cells = G ** 3
    bits = _build(logits.to(dev()), G, threshold, False)
    assert bits.numel() == (cells + 31) // 32
    got = _unpack(bits)
    assert not bool(got[cells:].any()), "bits past G^3 in the last word must be 0"
    decided, want = _build_expected(logits[:, 3], threshold)
    got = got[:cells]
    bad = decided & (got != want)
    assert not bool(bad.any()), "G=%d: %d cells decided against float64 softplus > %r, first %d (logit %r)" % (
        G, int(bad.sum()), threshold, int(bad.nonzero()[0, 0]), float(logits[int(bad.nonzero()[0, 0]), 3]))
    if G > 1:                           # (the data reaches both answers)
        assert 0 < int(want[decided].sum()) < int(decided.sum())
    ident = logits[:, 3] > 20.0
    if threshold > 20.0 and G > 1:      # the strict > on the identity branch: x == threshold is empty
        eq = ident & (logits[:, 3] == float(np.float32(threshold)))
        assert bool(eq.any()) and not bool(got[eq].any())
    # dilation of the kernel's own undilated bits, exactly
    dil = _unpack(_build(logits.to(dev()), G, threshold, True))
    assert not bool(dil[cells:].any()), "dilated bits past G^3 in the last word must be 0"
    exp = F.max_pool3d(got.reshape(1, 1, G, G, G).float(), 3, 1, 1).reshape(-1) > 0
    assert torch.equal(dil[:cells], exp)


# ----------------------------------------------------------------------------------- count / scan / compact
def _grid(G, lo, size, seed):
    logits = torch.randn((G ** 3, 4), generator=torch.Generator().manual_seed(seed)) * 2
    bits = ops.occupancy_build(logits.to(dev()), G, 0.7, False)
    return types.SimpleNamespace(resolution=G, box_min=lo, box_size=size, bits=bits)


def _samples(n, grid, seed):
    """Uniform in a box a bit larger than the grid's, then cell boundaries, box faces, NaN rows."""
    gen = torch.Generator().manual_seed(seed)
    lo = torch.tensor(grid.box_min, dtype=torch.float32)
    size = torch.tensor(grid.box_size, dtype=torch.float32)
    G = grid.resolution
    pos = lo + (torch.rand((n, 3), generator=gen) * 1.2 - 0.1) * size
    if n >= 64:
        k = torch.randint(0, G + 1, (n // 4, 3), generator=gen).float()
        pos[: n // 4] = lo + k * (size / G)              # cell boundaries, k = G on the top face
        pos[n // 4: n // 4 + 8] = lo                     # the lower box corner
        pos[n // 4 + 8: n // 4 + 16] = lo + size         # the upper one
        nan = torch.randint(0, n, (max(1, n // 50),), generator=gen)
        pos[nan, torch.randint(0, 3, nan.shape, generator=gen)] = float("nan")
    return pos.contiguous()


def _expected_occupied(grid, pos):
    occ = torch.zeros(pos.shape[0], dtype=torch.bool)
    fin = torch.isfinite(pos).all(1)
    occ[fin] = _cpu_occupied(grid, pos[fin])
    return occ | ~fin


@pytest.mark.parametrize("n,G,views", [(1, 5, True), (262143, 33, True), (262144, 64, False),
                                        (262145, 33, False), (3000017, 64, True)])
def test_count_scan_compact_exact(n, G, views):
    lo, size = (-1.0, -0.5, -2.0), (2.0, 1.0, 4.0)
    grid = _grid(G, lo, size, n)
    pos = _samples(n, grid, n + 1)
    view = torch.randn((n, 3), generator=torch.Generator().manual_seed(2)) if views else None
    occ = _expected_occupied(grid, pos)
    # the block counts and their exclusive scan (more than one count per scan thread above 262 144)
    blocks = (n + 255) // 256
    offsets = torch.full((blocks,), -7, dtype=torch.int32, device=dev())
    total = torch.full((1,), -7, dtype=torch.int64, device=dev())
    pos_d = pos.to(dev())
    ops._call("ffn_occupancy_count", ops._dev(pos_d), c_i64(n), ops._host3(lo), ops._host3(size), c_i(G),
              ops._dev(grid.bits, torch.int32), ops._dev(offsets, torch.int32), ops._dev(total, torch.int64))
    torch.cuda.synchronize()
    counts = torch.zeros(blocks * 256, dtype=torch.int64)
    counts[:n] = occ.long()
    counts = counts.reshape(blocks, 256).sum(1)
    assert int(total) == int(occ.sum())
    assert torch.equal(offsets.cpu().long(), torch.cumsum(counts, 0) - counts)
    pc, vc, index = ops.occupancy_compact(pos_d, view.to(dev()) if views else None, lo, size, G, grid.bits)
    exp_index = occ.nonzero().reshape(-1)
    assert torch.equal(index.cpu().long(), exp_index)
    assert torch.equal(pc.cpu().view(torch.int32), pos[exp_index].view(torch.int32))   # (NaN rows too)
    if views:
        assert torch.equal(vc.cpu(), view[exp_index])
    else:
        assert vc is None
    if n > 1:
        assert 0 < exp_index.numel() < n


# ----------------------------------------------------------------------------------- scatter / gather
@pytest.mark.parametrize("n", [1, 1000, 2 ** 21 + 5])
def test_scatter_gather_at_m_zero_and_n(n):
    gen = torch.Generator().manual_seed(n)
    fill = torch.tensor([0.0, 0.0, 0.0, -100.0])
    empty = torch.zeros((0,), dtype=torch.int32, device=dev())
    full = ops.scatter_logits(torch.zeros((0, 4), device=dev()), empty, n)
    assert torch.equal(full.cpu(), fill.expand(n, 4))
    assert ops.gather_logits(full, empty).shape == (0, 4)
    for index in (torch.arange(n, dtype=torch.int32), torch.randperm(n, generator=gen).int()):
        packed = torch.randn((n, 4), generator=gen)
        full = ops.scatter_logits(packed.to(dev()), index.to(dev()), n)
        exp = torch.empty((n, 4))
        exp[index.long()] = packed
        assert torch.equal(full.cpu(), exp)
        assert torch.equal(ops.gather_logits(full, index.to(dev())).cpu(), packed)
