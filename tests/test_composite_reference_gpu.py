"""The compositing and loss kernels against float64 with error budgets (tests/composite_reference.py).

Every launch goes straight through the C ABI with its output buffers filled with NaN, so an element a
kernel leaves unwritten fails.  Each case runs K5, K5b, K5w, K5w's backward (S <= 256), K6, K5t,
loss_from_partials and loss_value on rays of every regime of ``composite_reference.make_rays`` and
holds every element to ``kappa * 2^-24 * budget``; the deliberately changed references (teeth) must
fail.  The composite is f32 in every arithmetic mode, so the file runs unchanged under
``--precision bf16x6``."""

import json

import pytest
import torch

from fourier_feature_nets_amd import ops
from fourier_feature_nets_amd._lib import FfnError, c_f, c_i
from tests import composite_reference as cr

pytestmark = pytest.mark.gpu

SAMPLES = [1, 2, 63, 64, 65, 128, 129, 256, 257, 512]
RAYS = [1, 3, 257]
MANY_RAYS = 65541            # above 16384 rays (4096 workgroups of 4 waves) a wave takes several rays
ALPHA_WEIGHT = 0.1


def dev():
    return torch.device("cuda:0")


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev())


def _launch_composite(logits, t, d_colour, d_alpha):
    R, S = t.shape
    colour, alpha, depth = _nan(R, 3), _nan(R), _nan(R)
    flag = torch.zeros((1,), dtype=torch.int32, device=dev())
    ops._call("ffn_composite_fwd", ops._dev(logits), ops._dev(t), c_i(R), c_i(S), ops._dev(colour),
              ops._dev(alpha), ops._dev(depth), ops._dev(flag, torch.int32))
    d_logits = _nan(R, S, 4)
    ops._call("ffn_composite_bwd", ops._dev(logits), ops._dev(t), ops._dev(d_colour), ops._dev(d_alpha),
              c_i(R), c_i(S), ops._dev(d_logits))
    return colour, alpha, depth, d_logits, flag


def _launch_blend(t, sigma, d_weights):
    R, S = t.shape
    w = _nan(R, S)
    ops._call("ffn_blend_weights", ops._dev(t), ops._dev(sigma), c_i(R), c_i(S), ops._dev(w))
    if S > 256:
        return w, None, None
    d_sigma, d_t = _nan(R, S), _nan(R, S)
    ops._call("ffn_blend_weights_bwd", ops._dev(t), ops._dev(sigma), ops._dev(d_weights), c_i(R), c_i(S),
              ops._dev(d_sigma), ops._dev(d_t))
    return w, d_sigma, d_t


def _launch_mse(colour, alpha, gt_c, gt_a, ray_index, cs, as_):
    R = colour.shape[0]
    sums, d_colour, d_alpha = _nan(2), _nan(R, 3), _nan(R)
    scratch = _nan(2 * ((R + 255) // 256))
    ops._call("ffn_mse_loss", ops._dev(colour), ops._dev(alpha), ops._dev(gt_c), ops._dev(gt_a),
              ops._dev(ray_index, torch.int64), c_i(R), c_f(cs), c_f(as_), ops._dev(sums), ops._dev(d_colour),
              ops._dev(d_alpha), ops._dev(scratch))
    return sums, d_colour, d_alpha


def _launch_train(logits, t, gt_c, gt_a, ray_index, cs, as_, aw):
    R, S = t.shape
    blocks = cr.train_blocks(R)
    assert blocks == int(ops._lib.load().ffn_composite_train_blocks(c_i(R)))
    d_logits, partials = _nan(R, S, 4), _nan(blocks, 2)
    flag = torch.zeros((1,), dtype=torch.int32, device=dev())
    ops._call("ffn_composite_train", ops._dev(logits), ops._dev(t), c_i(R), c_i(S), ops._dev(gt_c),
              ops._dev(gt_a), ops._dev(ray_index, torch.int64), c_f(cs), c_f(as_), ops._dev(d_logits),
              ops._dev(partials), ops._dev(flag, torch.int32))
    sums, loss, loss2 = _nan(2), _nan(1), _nan(1)
    ops._call("ffn_loss_from_partials", ops._dev(partials), c_i(blocks), c_f(3.0 * R), c_f(float(R)), c_f(aw),
              ops._dev(sums), ops._dev(loss))
    ops._call("ffn_loss_value", ops._dev(sums), c_f(3.0 * R), c_f(float(R)), c_f(aw), ops._dev(loss2))
    return d_logits, partials, sums, loss, loss2, flag


def _case(R, S, with_alpha=True):
    seed = 1000 * S + R
    logits, t, sigma = (x.to(dev()) for x in cr.make_rays(R, S, seed))
    dc, da, dw = (x.to(dev()) for x in cr.make_grads(R, S, seed))
    gc, ga, idx = (x.to(dev()) for x in cr.make_truth(R, seed))
    if not with_alpha:
        ga = None
    cs, as_, aw = 1.0 / (3 * R), (ALPHA_WEIGHT / R if with_alpha else 0.0), (ALPHA_WEIGHT if with_alpha else 0.0)
    rep = cr.Report()
    key = "R=%d S=%d" % (R, S)

    colour, alpha, depth, d_logits, flag = _launch_composite(logits, t, dc, da)
    w, d_sigma, d_t = _launch_blend(t, sigma, dw)
    sums, d_colour, d_alpha = _launch_mse(colour, alpha, gc, ga, idx, cs, as_)
    d_logits_t, partials, sums_t, loss, loss2, flag_t = _launch_train(logits, t, gc, ga, idx, cs, as_, aw)
    torch.cuda.synchronize()
    assert int(flag.item()) == 0 and int(flag_t.item()) == 0, "NaN flag raised on finite inputs"

    cr.measure_composite(rep, key, logits, t, dc, da, colour, alpha, depth, d_logits)
    cr.measure_blend(rep, key, t, sigma, dw, w, d_sigma, d_t)
    cr.measure_mse(rep, key, colour, alpha, gc, ga, idx, cs, as_, sums, d_colour, d_alpha)
    cr.measure_train(rep, key, logits, t, gc, ga, idx, cs, as_, d_logits_t, partials)
    cr.measure_loss(rep, key, partials, R, aw, sums_t, loss, loss2)
    teeth = {k: (round(v["ratio"], 3), v["out"]) for k, v in rep.teeth.items()}
    print("composite reference", json.dumps(dict(R=R, S=S, worst=rep.worst, teeth=teeth)))
    # every regime is present from 7 rays on; one sample leaves nothing for the inner-sample teeth
    required = cr.TEETH if (R >= len(cr.REGIMES) and S > 1) else ()
    problems = rep.problems(required)
    assert not problems, "\n".join(problems)


@pytest.mark.parametrize("S", SAMPLES)
@pytest.mark.parametrize("R", RAYS)
def test_composite_kernels_against_float64(R, S):
    _case(R, S, with_alpha=R != 3)


def test_several_rays_per_wave_against_float64():
    _case(MANY_RAYS, 64)


def test_sample_counts_past_the_templates_are_refused():
    t = torch.zeros((1, 513), dtype=torch.float32, device=dev())
    logits = torch.zeros((1, 513, 4), dtype=torch.float32, device=dev())
    one = torch.zeros((1, 3), dtype=torch.float32, device=dev())
    idx = torch.zeros((1,), dtype=torch.int64, device=dev())
    with pytest.raises(FfnError, match="ffn_composite_bwd: num_samples > 512"):
        ops.composite_bwd(logits, t, one, one[:, 0].contiguous())
    with pytest.raises(FfnError, match="ffn_composite_train: num_samples > 512"):
        ops.composite_train(logits, t, one, None, idx, 1.0, 0.0)
    t257 = torch.zeros((1, 257), dtype=torch.float32, device=dev())
    with pytest.raises(FfnError, match="ffn_blend_weights_bwd: num_samples > 256"):
        ops.blend_weights_bwd(t257, t257, t257, want_dt=True)
