"""The stage-by-stage float64 checker (tests/layer_reference.py) on synthetic buffers, no GPU needed.

Planning-only programs give the chains and layouts; the slabs, dZ, logits and gradients a
forward / backward pair would leave are computed here in float64 from the models' weights
(rounded to f32 once, as a correctly rounded kernel would leave them) and written in the
documented slab layout by an encoder of this file's own.  The checker must
pass on them and fail when one swizzled position, one padded channel, one dZ row past n or one
gradient entry is changed."""

import math

import pytest
import torch

import fourier_feature_nets_amd as ffn
from fourier_feature_nets_amd.mlp_engine import MlpProgram
from oracle import ffn_oracle as orc
from tests import layer_reference as lr

N = 1000            # ragged: 31.25 blocks


def _model(kind):
    torch.manual_seed(5)
    if kind == "tiny":
        return ffn.MLP(3, 4, num_layers=2, num_channels=32)
    if kind == "positional96":
        return ffn.PositionalFourierMLP(3, 4, 5.5, num_channels=96)
    if kind == "nerf100":
        return ffn.NeRF(4, 100, 5, 6, 2, 3, [2], True)
    raise KeyError(kind)


def _oracle_logits(model, x, v):
    if hasattr(model, "opacity_out"):
        params = {k: t.detach().double() for k, t in model.state_dict().items()}
        return orc.OracleNeRF(params, sorted(model.skips), model.include_inputs)(x, v)
    a = None if model.a_values is None else model.a_values.detach().double()
    b = None if model.b_values is None else model.b_values.detach().double()
    return orc.OracleFourierMLP(a, b, [m.weight.detach().double() for m in model.layers],
                                [m.bias.detach().double() for m in model.layers])(x)


def _write_slab(flat, prog, blocks, slot, rows):
    """Encoder: ``rows`` (32 * blocks, C) of slot ``slot`` into ``flat`` -- per block C * 32
    floats, float4 ``[channel // 4][sample ^ ((channel // 4) & 15)]``."""
    ch, off = int(prog.fwd.slot_channels[slot]), int(prog.fwd.slot_offset[slot])
    base = off * blocks * 32
    for c in range(ch):
        q = c // 4
        for s in range(32):
            idx = base + torch.arange(blocks) * (ch * 32) + q * 128 + 4 * (s ^ (q & 15)) + c % 4
            flat[idx] = rows[s::32, c]


def _synthetic(kind):
    """(program, inputs, buffers) of one forward / backward pair computed in float64."""
    model = _model(kind)
    enc, specs = model._chain(torch.device("cpu"))
    prog = MlpProgram(enc, specs, torch.device("cpu"), planning_only=True)
    blocks = (N + 31) // 32
    pad = 32 * blocks
    torch.manual_seed(7)
    x = (torch.rand(N, 3) * 2 - 1).double()
    v = torch.nn.functional.normalize(torch.randn(N, 3), dim=1).double()
    d_logits = (torch.randn(N, 4) / math.sqrt(N)).float()
    f32 = lambda t: t.float().double()         # noqa: E731  (what a correctly rounded kernel stores)
    inputs = {0: x, 1: v}
    feats = {}
    for e, spec in enumerate(prog.encodings):
        cols = []
        if spec.num_freq:
            arg = spec.scale * (inputs[e] @ spec.b.double())
            cols += [spec.a.double() * torch.cos(arg), spec.a.double() * torch.sin(arg)]
        if spec.include_input:
            cols.append(inputs[e])
        feats[e] = f32(torch.cat(cols, 1))
    outs, ins = {}, {}
    logits = torch.zeros(N, 4, dtype=torch.float64)
    for i, sp in enumerate(prog.layers):
        parts = []
        if sp.act_in > 0:
            parts.append(outs[prog.producer_of[i]])
        if sp.enc_id is not None:
            parts.append(feats[sp.enc_id])
        a = ins[i] = torch.cat(parts, 1)
        z = a @ sp.weight.detach().double().T + sp.bias.detach().double()
        if sp.to_logits is None:
            outs[i] = f32(torch.relu(z) if sp.relu else z)
        else:
            logits[:, sp.to_logits[0]:sp.to_logits[0] + sp.to_logits[1]] = z
    want = _oracle_logits(model, x, v) if model.use_view else _oracle_logits(model, x, None)
    torch.testing.assert_close(logits, want.detach().double(), rtol=1e-6, atol=1e-6)
    dzs = {}
    dl = d_logits.double()
    for j in reversed(range(len(prog.layers))):
        sp = prog.layers[j]
        if sp.to_logits is not None:
            dzs[j] = dl[:, sp.to_logits[0]:sp.to_logits[0] + sp.to_logits[1]]
            continue
        acc = torch.zeros(N, sp.out, dtype=torch.float64)
        for c, p in enumerate(prog.producer_of):
            if p == j:
                acc += dzs[c] @ prog.layers[c].weight.detach().double()[:, :sp.out]
        dzs[j] = f32(acc * (outs[j] > 0) if sp.relu else acc)
    grads = torch.zeros(prog.num_grad_floats, dtype=torch.float32)
    for i, sp in enumerate(prog.layers):
        grads[prog.grad_w_off[i]:prog.grad_w_off[i] + sp.out * sp.ld] = (dzs[i].T @ ins[i]).reshape(-1).float()
        grads[prog.grad_b_off[i]:prog.grad_b_off[i] + sp.out] = dzs[i].sum(0).float()
    saved = torch.zeros(prog.saved_floats(N), dtype=torch.float32)
    dz = torch.zeros(prog.dz_channels * 32 * blocks, dtype=torch.float32)

    def padded_rows(values, width, past_n_like_last):
        rows = torch.zeros(pad, width, dtype=torch.float32)
        rows[:N, :values.shape[1]] = values.float()
        if past_n_like_last:          # the kernels' tail lanes recompute the last sample
            rows[N:, :values.shape[1]] = values[-1].float()
        return rows

    for j, slot in prog.slot_of.items():
        _write_slab(saved, prog, blocks, slot, padded_rows(outs[j], prog.layers[j].out_p, True))
        _write_slab(dz, prog, blocks, slot, padded_rows(dzs[j], prog.layers[j].out_p, False))
    for e, slot in prog.enc_slot.items():
        spec = prog.encodings[e]
        internal = torch.zeros(N, spec.width, dtype=torch.float64)
        for c in range(spec.width):
            if spec.natural_index(c) >= 0:
                internal[:, c] = feats[e][:, spec.natural_index(c)]
        _write_slab(saved, prog, blocks, slot, padded_rows(internal, spec.width, True))
    return prog, dict(positions=x.float(), views=v.float() if model.use_view else None, saved=saved,
                      dz=dz, d_logits=d_logits, logits=logits.float(), grads=grads)


KINDS = ["tiny", "positional96", "nerf100"]


@pytest.fixture(scope="module", params=KINDS)
def synthetic(request):
    return _synthetic(request.param)


def _measure(prog, b):
    return lr.measure_layers(prog, b["positions"], b["views"], b["saved"], b["dz"], b["d_logits"],
                             b["logits"], b["grads"])


def test_checker_passes_on_correctly_rounded_buffers(synthetic):
    prog, b = synthetic
    report = lr.check_layers(prog, b["positions"], b["views"], b["saved"], b["dz"], b["d_logits"],
                             b["logits"], b["grads"])
    for stage, (worst, teeth) in report.items():
        if stage == "logits" and not any(sp.to_logits for sp in prog.layers):
            continue
        # one rounding to f32 of the result (or of every input): well inside every kappa
        assert worst <= 3.0 and teeth > lr.KAPPA["f32"][stage], (stage, worst, teeth)
    # slab_rows keeps its shape on top of slot_rows; dz_rows returns the padding and the rows past n too
    j = max(prog.slot_of)
    assert prog.slab_rows(b["saved"], N, j).shape == (N, prog.layers[j].out)
    assert prog.dz_rows(b["dz"], N, j).shape == (32 * ((N + 31) // 32), prog.layers[j].out_p)


def _swap_positions(b, prog):
    """Swaps samples 0 and 1 of the first channel quad of the first hidden slab where they differ
    (one swizzle wrong)."""
    slot = min(prog.slot_of.values())
    ch, off = int(prog.fwd.slot_channels[slot]), int(prog.fwd.slot_offset[slot])
    blocks = (N + 31) // 32
    for q in range(ch // 4):
        base = off * blocks * 32 + q * 128
        p, r = 4 * (0 ^ (q & 15)), 4 * (1 ^ (q & 15))
        first, second = b["saved"][base + p:base + p + 4].clone(), b["saved"][base + r:base + r + 4].clone()
        if not torch.equal(first, second):
            b["saved"][base + p:base + p + 4] = second
            b["saved"][base + r:base + r + 4] = first
            return
    raise AssertionError("no two different samples")


def _padded_channel(b, prog):
    """A non-zero value in a padded channel (a hidden slab if a width is padded, else a feature slab)."""
    blocks = (N + 31) // 32
    for j, slot in prog.slot_of.items():
        if prog.layers[j].out_p > prog.layers[j].out:
            c = prog.layers[j].out
            break
    else:
        e, slot = next(iter(prog.enc_slot.items()))
        c = [k for k in range(prog.encodings[e].width) if prog.encodings[e].natural_index(k) < 0][0]
    off = int(prog.fwd.slot_offset[slot])
    ch = int(prog.fwd.slot_channels[slot])
    q = c // 4
    b["saved"][off * blocks * 32 + 3 * ch * 32 + q * 128 + 4 * (5 ^ (q & 15)) + c % 4] = 1e-3


def _dz_row_past_n(b, prog):
    blocks = (N + 31) // 32
    slot = min(prog.slot_of.values())
    off, ch = int(prog.fwd.slot_offset[slot]), int(prog.fwd.slot_channels[slot])
    s = N % 32 + 2                        # a row of the last block past n
    b["dz"][off * blocks * 32 + (blocks - 1) * ch * 32 + 4 * (s ^ 0)] = 1e-6


def _gradient_entry(b, prog):
    i = 0
    sp = prog.layers[i]
    g = b["grads"][prog.grad_w_off[i]:prog.grad_w_off[i] + sp.out * sp.ld]
    k = int(g.abs().argmax())
    g[k] += 1e-4 * float(g.abs().max())


@pytest.mark.parametrize("mutate,expect", [(_swap_positions, "layers"), (_padded_channel, "padded"),
                                           (_dz_row_past_n, "past n"), (_gradient_entry, "weights")])
def test_checker_fails_on_one_wrong_value(synthetic, mutate, expect):
    prog, clean = synthetic
    b = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in clean.items()}
    mutate(b, prog)
    _, problems = _measure(prog, b)
    assert problems and any(expect in p for p in problems), problems


def test_inference_check_holds_the_bits_and_bounds_only_reordered_rows(synthetic, monkeypatch):
    """``check_inference`` on a stand-in inference launch: equal bits pass; one last-place change
    fails; past ``reordered_from`` a change within the logits head's rounding budget passes and is
    reported, one beyond it (a hidden layer that differs) fails."""
    prog, b = synthetic
    if not any(sp.to_logits for sp in prog.layers):
        return
    train = b["logits"]
    out = {}
    monkeypatch.setattr(prog, "forward", lambda x, views, saved, precision="f32": out["logits"], raising=False)
    args = (prog, b["positions"], b["views"], train, "f32")
    out["logits"] = train.clone()
    got, worst = lr.check_inference(*args)
    assert torch.equal(got, train) and worst == 0.0
    _, terms = lr._logits_head(prog, b["saved"], N)
    row = N - 5
    col = int(terms[row].argmax())
    ulp = train.clone()
    ulp[row, col] = torch.nextafter(ulp[row, col], torch.tensor(float("inf")))
    out["logits"] = ulp
    with pytest.raises(AssertionError, match="differ from the training forward"):
        lr.check_inference(*args, saved=b["saved"])
    with pytest.raises(AssertionError, match="differ from the training forward"):
        lr.check_inference(*args, saved=b["saved"], reordered_from=row + 1)
    _, worst = lr.check_inference(*args, saved=b["saved"], reordered_from=row)
    assert 0.0 < worst <= lr.KAPPA["f32"]["logits"]
    far = train.clone()
    far[row, col] += float(2 * lr.KAPPA["f32"]["logits"] * lr.U * terms[row, col])
    out["logits"] = far
    with pytest.raises(AssertionError, match="hidden layers differ"):
        lr.check_inference(*args, saved=b["saved"], reordered_from=row)
