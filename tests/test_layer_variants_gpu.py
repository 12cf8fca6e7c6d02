"""The fused-MLP kernels the default training launch never reaches, against float64 stage by stage.

``tests/test_layer_reference_gpu.py`` holds every stage of the training forward and backward to
``kappa * 2^-24 * sum|terms|`` -- in whichever organisation the launcher picks by default.  This file
runs the same check (``_run`` -> ``layer_reference.check_layers``, teeth included, the kappa of the
precision as it stands) on what that leaves out:

1. every selectable organisation: the split-bf16 ring kernels (forward AND backward data), the
   two-waves-per-SIMD kernels with polynomial / hardware sin and cos and 8 / 16 waves, the bf16x6
   chains on the two-waves-per-SIMD kernels, with nine products and with two forward accumulators,
   and the exact-f32 launches without their tail on wave teams;
2. inference launches (``saved=None``): bit for bit the training forward's logits of the same
   organisation, independent of the batch around a row, and which kernel the default split-bf16
   inference launch runs;
3. angles up to the 5000 rad the sin / cos routines document (quadrant counts in the thousands).
"""

import ctypes
import json

import pytest
import torch

from fourier_feature_nets_amd import _lib, mlp_engine
from tests import layer_reference as lr
from tests import test_layer_reference_gpu as ref
from tests.test_layer_reference_gpu import CHAINS, MODES, _inputs, _model, _run, _sizes, dev

pytestmark = pytest.mark.gpu

WIDE = ["gaussian512", "nerf512", "nerf1024", "mlp768"]       # split-bf16: two-waves-per-SIMD kernels only; no bf16x6
BIG = ["nerf1024", "mlp768"]                                   # beyond 512 channels: exact f32 only, bf16x3 refuses them too
NARROW = [c for c in CHAINS if c not in WIDE]
# several passes of four blocks, a partial pass, a partial block
SIZES = [1000, 4 * 32 * 3 + 45]
SIZE_CHAINS = ["positional", "nerf_small", "mlp96"]            # the chains of the planner's size test
assert set(m.split("+")[0] for m in MODES) == {"f32", "bf16x6", "bf16x3"}

BF16X3_SWITCHES = ("FFN_BF16_KERNELS", "FFN_BF16_SINCOS", "FFN_BF16_WAVES")
BF16X3_ORGS = {
    "ring": dict(FFN_BF16_KERNELS="ring"),
    "ws-poly-8": dict(FFN_BF16_KERNELS="ws", FFN_BF16_SINCOS="poly", FFN_BF16_WAVES="8"),
    "ws-hw-16": dict(FFN_BF16_KERNELS="ws", FFN_BF16_SINCOS="hw", FFN_BF16_WAVES="16"),
    "ws-poly-16": dict(FFN_BF16_KERNELS="ws", FFN_BF16_SINCOS="poly", FFN_BF16_WAVES="16"),
    # ws-hw-8 is what a training launch runs by default: test_layer_reference_gpu.py
    "ws": dict(FFN_BF16_KERNELS="ws"),                # (inference: the default's sin / cos and waves)
    "ws-hw-8": dict(FFN_BF16_KERNELS="ws", FFN_BF16_SINCOS="hw", FFN_BF16_WAVES="8"),
    "default": dict(),
}
BF16X6_SWITCHES = ("FFN_BF16X6_ORG", "FFN_BF16X6_PRODUCTS", "FFN_BF16X6_FWD_ACCS")
BF16X6_ORGS = {
    "ws": dict(FFN_BF16X6_ORG="ws"),
    "products9": dict(FFN_BF16X6_PRODUCTS="9"),
    "accs2": dict(FFN_BF16X6_FWD_ACCS="2"),
    "default": dict(),
}


def _select(monkeypatch, switches, values):
    """The launcher reads its switches with getenv at every launch."""
    for k in switches:
        monkeypatch.delenv(k, raising=False)
    for k, v in values.items():
        monkeypatch.setenv(k, v)


def _select_org(monkeypatch, org):
    """``org``: "f32" | "bf16x6" | "bf16x6-<BF16X6_ORGS key>" | "bf16x3-<BF16X3_ORGS key>"; returns
    the precision."""
    precision, _, variant = org.partition("-")
    _select(monkeypatch, BF16X3_SWITCHES, BF16X3_ORGS[variant or "default"] if precision == "bf16x3" else {})
    _select(monkeypatch, BF16X6_SWITCHES, BF16X6_ORGS[variant or "default"] if precision == "bf16x6" else {})
    return precision


def _x6_query(prog, backward=False):
    """`ffn_mlp_bf16x6_organisation`: 1 = matrix / vector waves, 0 = two waves per SIMD."""
    fn = _lib.load().ffn_mlp_bf16x6_organisation
    fn.restype = ctypes.c_int
    return int(fn(ctypes.byref(prog.bwd_x6 if backward else prog.fwd_x6), ctypes.c_int(1 if backward else 0)))


def _report(capsys):
    """The report of the `layer reference {...}` line ``_run`` printed last (printed again: capsys
    took it)."""
    out = capsys.readouterr().out
    print(out, end="")
    lines = [ln for ln in out.splitlines() if ln.startswith("layer reference ")]
    assert lines, "no `layer reference` line"
    return json.loads(lines[-1][len("layer reference "):])["report"]


# ------------------------------------------------------------------ 1. every organisation, stage by stage
def _bf16x3_cases():
    cases = [(name, org, n) for name in NARROW for org in ("ring", "ws-poly-8", "ws-hw-16", "ws-poly-16")
             for n in SIZES]
    # 512-wide chains exist only as two-waves-per-SIMD kernels with their own shape (no 16-wave
    # variant): the polynomial request, and a ring request that must fall back; the chains beyond
    # 512 channels have no split-bf16 kernels and must be refused under every switch
    cases += [(name, org, n) for name in WIDE for org in ("ring", "ws-poly-8") for n in SIZES]
    return cases


@pytest.mark.parametrize("name,org,n", _bf16x3_cases())
def test_split_bf16_organisations_stage_by_stage(name, org, n, monkeypatch):
    """bf16x3 under every value of FFN_BF16_KERNELS / FFN_BF16_SINCOS / FFN_BF16_WAVES but the
    default's: forward slabs, logits, dZ (the ring backward of mlp_bf16_bwd.hip included) and the
    gradients computed from them, against float64 within the mode's kappa."""
    _select(monkeypatch, BF16X3_SWITCHES, BF16X3_ORGS[org])
    prog = _run(name, n, "bf16x3", monkeypatch)
    assert (prog is not None) == _model(name).program().covers("bf16x3")
    if name in WIDE:
        assert (prog is None) == (name in BIG)


def _train_logits(name, n, precision):
    model = _model(name)
    prog = model.program()
    x, views, _ = _inputs(model, n)
    saved = torch.full((prog.saved_floats(n),), float("nan"), device=dev())
    logits = prog.forward(x, views, saved, precision=precision)
    assert bool(torch.isfinite(logits).all())
    return prog, x, views, saved, logits


def test_ring_request_selects_other_kernels_than_ws(monkeypatch):
    """There is no query for which split-bf16 kernels ran.  The two organisations add the fused
    heads' partial sums in different orders, so on the same polynomial features their training
    logits must differ in some bit for at least one narrow chain -- else FFN_BF16_KERNELS did
    nothing; on the wide chains, where a ring request falls back, they must not differ at all."""
    differ = {}
    for name in CHAINS:
        if not _model(name).program().covers("bf16x3"):
            continue
        out = {}
        for org in ("ring", "ws-poly-8"):
            _select(monkeypatch, BF16X3_SWITCHES, BF16X3_ORGS[org])
            out[org] = _train_logits(name, 1000, "bf16x3")[4]
        differ[name] = not torch.equal(out["ring"].view(torch.int32), out["ws-poly-8"].view(torch.int32))
    print("ring != ws (training logits, any bit)", json.dumps(differ))
    assert all((name in differ) == (name not in BIG) for name in WIDE)
    assert not any(differ[name] for name in WIDE if name not in BIG), differ
    assert any(v for name, v in differ.items() if name not in WIDE), differ


def _bf16x6_cases():
    return [(name, org, n) for name in NARROW for org in ("ws", "products9", "accs2") for n in SIZES]


@pytest.mark.parametrize("name,org,n", _bf16x6_cases())
def test_bf16x6_organisations_stage_by_stage(name, org, n, monkeypatch):
    """bf16x6 under FFN_BF16X6_ORG=ws, FFN_BF16X6_PRODUCTS=9 and FFN_BF16X6_FWD_ACCS=2, one at a
    time, within the exact kernels' kappa; the launcher's own query confirms what the case runs."""
    prog = _model(name).program()
    assert prog.covers("bf16x6")
    _select(monkeypatch, BF16X6_SWITCHES, {})
    by_default = _x6_query(prog)
    if name == "positional":            # the tiny NeRF / Fourier MLP family: matrix / vector waves
        assert by_default == 1 and _x6_query(prog, backward=True) == 1
    _select(monkeypatch, BF16X6_SWITCHES, BF16X6_ORGS[org])
    assert _x6_query(prog) == 0
    if org != "accs2":                  # (two forward accumulators: a switch of the forward alone)
        assert _x6_query(prog, backward=True) == 0
    print("bf16x6 organisation", json.dumps(dict(chain=name, default=by_default, org=org)))
    assert _run(name, n, "bf16x6", monkeypatch) is not None


@pytest.mark.parametrize("label", ["tail-quads", "tail-pairs"])
@pytest.mark.parametrize("off", ["TAIL_PAIRS", "TAIL_QUADS"])
@pytest.mark.parametrize("name", SIZE_CHAINS)
def test_exact_f32_without_wave_teams_stage_by_stage(name, off, label, monkeypatch):
    """The exact-f32 launches whose tail the planner would put on teams of four (``TAIL_QUADS``) or
    two (``TAIL_PAIRS``) waves, with that switched off: the one-wave-per-block kernels on every block,
    or pairs where quads would run.  ``quad_chain_ok`` is fixed when the program is built, so the
    model is built inside the test."""
    monkeypatch.setattr(mlp_engine, off, False)
    monkeypatch.setattr(ref, "_MODELS", {})           # `_model` and `_run` build and share a fresh one
    prog = _model(name).program()
    n = dict(_sizes(prog))[label]
    plan = prog._tail_plan(n)
    if off == "TAIL_PAIRS" or not prog.pair_chain_ok:
        assert plan is None
    else:
        assert not prog.quad_chain_ok and plan is not None and plan[1] == 2
    assert _run(name, n, "f32", monkeypatch) is prog


# ------------------------------------------------------------------ 2. inference launches
INFERENCE_ORGS = ["f32", "bf16x6", "bf16x6-ws", "bf16x3-ring", "bf16x3-ws"]
INFERENCE_SIZES = ["one", "31", "33", "tail-quads", "tail-pairs", "plan-step"]


def _inference(name, n, org, monkeypatch):
    precision = _select_org(monkeypatch, org)
    prog = _model(name).program()
    if not prog.covers(precision):
        x, views, _ = _inputs(_model(name), n)
        with pytest.raises(NotImplementedError):
            prog.forward(x, views, None, precision=precision)
        return None
    prog, x, views, saved, logits = _train_logits(name, n, precision)
    # the exact-f32 TRAINING launch puts a short last round on teams of waves, which add a fused
    # head's partial products in another order (mlp_engine.py, above TAIL_PAIRS); inference never does
    plan = prog._tail_plan(n) if precision == "f32" else None
    cut = None if plan is None else 32 * plan[0]
    got, worst = lr.check_inference(prog, x, views, logits, precision, saved=saved, reordered_from=cut)
    assert bool(torch.isfinite(got).all())
    print("inference", json.dumps(dict(chain=name, n=n, org=org, bit_equal=worst == 0.0, team_rows_from=cut,
                                       worst_ratio=worst)))
    return got


@pytest.mark.parametrize("org", INFERENCE_ORGS)
@pytest.mark.parametrize("name", CHAINS)
def test_inference_launch_equals_the_training_forward(name, org, monkeypatch):
    """``prog.forward(x, views, None)`` -- what voxelize, bake and every render call -- on every chain
    in every organisation: the bits of the training forward's logits, which
    test_layer_reference_gpu.py and the tests above hold to float64."""
    _inference(name, 1000, org, monkeypatch)


@pytest.mark.parametrize("label", INFERENCE_SIZES)
@pytest.mark.parametrize("org", INFERENCE_ORGS)
@pytest.mark.parametrize("name", SIZE_CHAINS)
def test_inference_launch_at_the_planner_sizes(name, org, label, monkeypatch):
    """One sample, either side of a block, a rounded-up plan and the two sizes whose exact-f32
    TRAINING launch runs its last round on teams of waves (there the rows of that round are held to
    the logits head's rounding budget, every other row to the bits)."""
    n = dict(_sizes(_model(name).program()))[label]
    assert _inference(name, n, org, monkeypatch) is not None
    prog = _model(name).program()
    if org == "f32" and label.startswith("tail") and prog.pair_chain_ok:
        assert prog._tail_plan(n) is not None


@pytest.mark.parametrize("name", CHAINS)
def test_default_split_bf16_inference_is_one_of_the_two_organisations(name, monkeypatch):
    """Which kernel renders in bf16x3: without a switch the inference launch must write the bits of
    the ring or of the two-waves-per-SIMD inference launch."""
    model = _model(name)
    prog = model.program()
    if not prog.covers("bf16x3"):
        return
    x, views, _ = _inputs(model, 1000)
    out = {}
    for org in ("default", "ring", "ws"):
        _select(monkeypatch, BF16X3_SWITCHES, BF16X3_ORGS[org])
        out[org] = prog.forward(x, views, None, precision="bf16x3").view(torch.int32)
    ran = [org for org in ("ring", "ws") if torch.equal(out["default"], out[org])]
    print("default bf16x3 inference", json.dumps(dict(chain=name, equals=ran)))
    assert ran, "the default inference launch equals neither organisation"
    if name in WIDE:
        assert ran == ["ring", "ws"]        # (a ring request falls back)


@pytest.mark.parametrize("n", [33, 1000])
@pytest.mark.parametrize("org", ["f32", "bf16x6", "bf16x6-ws", "bf16x3", "bf16x3-ring", "bf16x3-ws"])
@pytest.mark.parametrize("name", ["positional", "nerf_small"])
def test_inference_rows_do_not_depend_on_the_batch(name, org, n, monkeypatch):
    """Rows 0 .. n-1 inside a batch of n + 37 come out with the bits they have in a batch of n."""
    precision = _select_org(monkeypatch, org)
    model = _model(name)
    prog = model.program()
    x, views, _ = _inputs(model, n + 37)
    big = prog.forward(x, views, None, precision=precision)
    small = prog.forward(x[:n].contiguous(), None if views is None else views[:n].contiguous(), None,
                         precision=precision)
    assert bool(torch.isfinite(big).all())
    assert torch.equal(big[:n].view(torch.int32), small.view(torch.int32))


# ------------------------------------------------------------------ 3. angles up to the documented limit
ANGLE_TARGET = 4500.0
ANGLE_ORGS = ["f32", "bf16x6", "bf16x3-ws-poly-8", "bf16x3-ws-hw-8", "bf16x3-ring"]


@pytest.mark.parametrize("org", ANGLE_ORGS)
@pytest.mark.parametrize("name", ["positional", "gaussian", "nerf"])
def test_angles_up_to_the_documented_limit(name, org, monkeypatch, capsys):
    """Positions uniform in [-r, r]^3 with r chosen, in float64, so that the largest |scale x.B| of
    the batch is about 4500 rad (common.h and bf16_ring.h state their sin / cos "for |x| <= 5000";
    positions in the unit box stop near 800): quadrant counts in the thousands and a reduction by
    2 pi of a few hundred turns.  The same budget |a| (s sum|x_d B_dk| + 1) -- at these angles the
    rounding of the angle dominates it, so the last ulp of a polynomial is not seen, a wrong
    quadrant or a broken reduction (O(1)) is."""
    precision = _select_org(monkeypatch, org)
    model = _model(name)
    prog = model.program()
    enc = prog.encodings[0]
    assert enc.num_freq > 0
    n = 1000
    b = enc.b.double().cpu()

    def largest(radius):
        x = _inputs(model, n, radius=radius)[0].double().cpu()
        return float((float(enc.scale) * (x @ b)).abs().max())

    r = ANGLE_TARGET / largest(1.0)
    top = largest(r)
    print("angles", json.dumps(dict(chain=name, org=org, radius=r, largest_angle=top)))
    assert 4000.0 <= top <= 5000.0
    assert _run(name, n, precision, monkeypatch, radius=r) is not None
    worst, teeth = _report(capsys)["features"]
    assert teeth > lr.kappa_of(precision)["features"] >= worst
