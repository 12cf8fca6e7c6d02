"""Every fused-MLP kernel stage against float64 on its own inputs (tests/layer_reference.py).

``prog.forward`` / ``prog.backward`` are driven directly; the checker then reads the slabs, the dZ
workspace, the logits and the flat gradients and holds every element of every stage to
``kappa * 2^-24 * sum|terms|``.  The training buffer, the dZ workspace and the gradient buffer are
filled with NaN first: a slab, dZ row or gradient a kernel leaves unwritten -- or a dZ row past n,
or a block past the real count of a rounded-up plan, that reaches a gradient -- shows up as NaN."""

import json
import math
import os

import numpy as np
import pytest
import torch

from fourier_feature_nets_amd.mlp_engine import BIAS_LDS_FLOATS, MlpProgram
from tests import layer_reference as lr

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN_CHAINS = ["mlp", "basic", "positional", "gaussian", "gaussian512", "nerf", "nerf_small"]
MADE_CHAINS = ["mlp96", "nerf100", "mlp7", "nerf512", "nerf1024", "mlp768"]
# the narrow input windows of test_weight_gradients_of_narrow_input_windows: every (quadrants, fold)
FOLD_CHAINS = ["fold%d_%d" % cf for cf in [(256, 10), (256, 4), (128, 10), (128, 4), (64, 2), (256, 1)]]
CHAINS = GOLDEN_CHAINS + MADE_CHAINS + FOLD_CHAINS
MODES = ["f32", "bf16x6", "bf16x6+f32wgrad", "bf16x3"]
HEADLINE = 65536 * 64
_MODELS = {}


def dev():
    return torch.device("cuda:0")


def _model(name):
    if name in _MODELS:
        return _MODELS[name]
    import fourier_feature_nets_amd as ffn
    from tests.test_kernels_gpu import _load_fourier, _load_nerf
    from tests.test_round4_gpu import _make
    if name in GOLDEN_CHAINS:
        g = np.load(os.path.join(GOLDEN, "models.npz"), allow_pickle=False)
        if name.startswith("nerf"):
            model, _ = _load_nerf(g, name, [4] if name == "nerf" else [2], name == "nerf")
        else:
            model, _ = _load_fourier(g, name)
    elif name.startswith("fold"):
        channels, freqs = (int(v) for v in name[4:].split("_"))
        torch.manual_seed(channels + freqs)
        b = torch.randn(3, 3 * freqs) * 2.0
        model = ffn.FourierFeatureMLP(3, 4, torch.ones(3 * freqs), b, [channels] * 3)
    else:
        model = _make(name)
    model = model.to(dev())
    _MODELS[name] = model
    return model


def _inputs(model, n, seed=0, radius=1.0):
    """(positions uniform in [-radius, radius]^3, unit view directions or None, d(loss)/d(logits))
    of ``n`` samples: what ``_run`` feeds the kernels."""
    gen = torch.Generator(device=dev()).manual_seed(seed + n)
    x = (torch.rand(n, 3, device=dev(), generator=gen) * 2 - 1) * radius
    views = None
    if model.use_view:
        views = torch.nn.functional.normalize(torch.randn(n, 3, device=dev(), generator=gen), dim=1)
    d_logits = torch.randn(n, 4, device=dev(), generator=gen) / math.sqrt(n)
    return x, views, d_logits


def _run(name, n, mode, monkeypatch, seed=0, radius=1.0):
    """One forward / backward pair of ``n`` samples in ``mode``, checked stage by stage."""
    model = _model(name)
    prog = model.program()
    precision = mode.split("+")[0]
    monkeypatch.setenv("FFN_BF16X6_WGRAD", "f32" if mode == "bf16x6+f32wgrad" else "bf16x6")
    x, views, d_logits = _inputs(model, n, seed, radius)
    saved = torch.full((prog.saved_floats(n),), float("nan"), device=dev())
    if not prog.covers(precision):
        with pytest.raises(NotImplementedError):
            prog.forward(x, views, saved, precision=precision)
        return None
    logits = prog.forward(x, views, saved, precision=precision)
    ws = prog.workspace(n)
    ws.dz
    prog._dz.fill_(float("nan"))          # the whole grow-only buffer, past the plan's blocks too
    grads = torch.full((prog.num_grad_floats,), float("nan"), device=dev())
    prog.backward(d_logits, x, views, saved, grads, precision=precision)
    report = lr.check_layers(prog, x, views, saved, ws.dz, d_logits, logits, grads,
                             precision=precision, teeth=n >= 1000)
    print("layer reference", json.dumps(dict(chain=name, n=n, mode=mode, report=report)))
    return prog


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", CHAINS)
def test_every_chain_and_mode_stage_by_stage(name, mode, monkeypatch):
    """Ragged 1000 samples (31.25 blocks) on every chain family in every mode; a mode that has
    no kernels for a chain refuses it."""
    prog = _run(name, 1000, mode, monkeypatch)
    wide = name in ("gaussian512", "nerf512", "nerf1024", "mlp768")
    if mode == "f32" or (mode.startswith("bf16x6") and not wide):
        assert prog is not None
    if mode.startswith("bf16x6") and wide:
        assert prog is None
    if name == "nerf512":
        assert _model(name).program().fwd.bias_floats > BIAS_LDS_FLOATS     # bias beyond the LDS copy


def _sizes(prog):
    """Batch sizes derived from the planner: (label, n)."""
    waves = prog._resident_waves()
    out = [("one", 1), ("31", 31), ("33", 33)]
    # one round of one-wave blocks plus a tail of waves / 8 blocks (four-wave teams) and of
    # 3 waves / 8 blocks (wave pairs), ragged
    out.append(("tail-quads", 32 * (waves + waves // 8) - 5))
    out.append(("tail-pairs", 32 * (waves + 3 * waves // 8) - 9))
    # a block count one above a rounding step of plan_blocks (the plan covers blocks past the real ones)
    blocks = 4096 + 1
    assert MlpProgram.plan_blocks(32 * blocks) > blocks
    out.append(("plan-step", 32 * blocks - 3))
    # several segments, each of several blocks, per weight-gradient unit
    n = 40000 + 13
    raw = prog._plan_wgrad(MlpProgram.plan_blocks(n), "f32")
    segs = [s for _, launch, _ in raw["launches"] for s in launch]
    per_unit = {}
    for s in segs:
        per_unit.setdefault(s.job, []).append(s.blk_end - s.blk_begin)
    assert max(len(v) for v in per_unit.values()) >= 2
    assert max(max(v) for v in per_unit.values()) >= 2
    out.append(("segments", n))
    return out


SIZE_LABELS = ["one", "31", "33", "tail-quads", "tail-pairs", "plan-step", "segments"]


@pytest.mark.parametrize("label", SIZE_LABELS)
@pytest.mark.parametrize("mode", ["f32", "bf16x6", "bf16x3"])
@pytest.mark.parametrize("name", ["positional", "nerf_small", "mlp96"])
def test_batch_sizes_from_the_planner_stage_by_stage(name, mode, label, monkeypatch):
    prog = _model(name).program()
    n = dict(_sizes(prog))[label]
    if mode == "f32" and label.startswith("tail") and prog.pair_chain_ok:
        plan = prog._tail_plan(n)
        assert plan is not None and plan[1] == (4 if label == "tail-quads" and prog.quad_chain_ok else 2)
    assert _run(name, n, mode, monkeypatch) is not None


@pytest.mark.parametrize("mode", ["f32", "bf16x6"])
def test_headline_launch_stage_by_stage(mode, monkeypatch):
    """The benchmark's launch: 65 536 rays x 64 samples (slab offsets in floats past 2^31)."""
    prog = _model("positional").program()
    assert prog.saved_channels * HEADLINE > 2 ** 31
    try:
        assert _run("positional", HEADLINE, mode, monkeypatch) is not None
    finally:
        prog.release_workspaces()
        torch.cuda.empty_cache()
