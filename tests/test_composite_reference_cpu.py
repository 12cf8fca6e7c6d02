"""The float64 compositing / loss checker (tests/composite_reference.py) on a float32 CPU evaluation
of the same formulas, no GPU needed: the oracle's ``render`` / ``blend_weights`` / ``mse_loss`` and
their autograd.  The checker must pass on them, every deliberately changed reference must fail on
them, and one wrong element must fail."""

import pytest
import torch

from oracle import ffn_oracle as orc
from tests import composite_reference as cr

R = 257
SAMPLES = [2, 64, 65, 130, 257]      # (the oracle, like the reference, has no weights at S = 1)


def _evaluate(S):
    """The oracle's outputs of one batch of every regime, with the inputs."""
    seed = 7 * S
    logits, t, sigma = cr.make_rays(R, S, seed)
    dc, da, dw = cr.make_grads(R, S, seed)
    gc, ga, idx = cr.make_truth(R, seed)
    lg = logits.clone().requires_grad_(True)
    colour, alpha, depth = orc.render(lg, t, True)
    ((colour * dc).sum() + (alpha * da).sum()).backward()
    tt, sg = t.clone().requires_grad_(True), sigma.clone().requires_grad_(True)
    w = orc.blend_weights(tt, sg)
    (w * dw).sum().backward()
    # K6 on the rendered colour / alpha, in float32
    c, a = colour.detach(), alpha.detach()
    gcol, galpha = orc.ground_truth(gc, ga, idx)
    cs, as_ = 1.0 / (3 * R), 0.1 / R
    sums = torch.stack([(c - gcol).square().sum(), (a - galpha).square().sum()])
    loss = sums[0] / (3.0 * R) + 0.1 * (sums[1] / R)
    return dict(logits=logits, t=t, sigma=sigma, dc=dc, da=da, dw=dw, gc=gc, ga=ga, idx=idx, cs=cs, as_=as_,
                colour=c, alpha=a, depth=depth, d_logits=lg.grad, w=w.detach(), d_sigma=sg.grad, d_t=tt.grad,
                sums=sums, loss=loss.reshape(1), d_colour=(c - gcol) * (2 * cs), d_alpha=(a - galpha) * (2 * as_))


@pytest.fixture(scope="module", params=SAMPLES)
def batch(request):
    return request.param, _evaluate(request.param)


def _measure(b, teeth=True):
    rep = cr.Report()
    cr.measure_composite(rep, "oracle", b["logits"], b["t"], b["dc"], b["da"], b["colour"], b["alpha"],
                         b["depth"], b["d_logits"], teeth=teeth)
    cr.measure_blend(rep, "oracle", b["t"], b["sigma"], b["dw"], b["w"], b["d_sigma"], b["d_t"], teeth=teeth)
    cr.measure_mse(rep, "oracle", b["colour"], b["alpha"], b["gc"], b["ga"], b["idx"], b["cs"], b["as_"],
                   b["sums"], b["d_colour"], b["d_alpha"])
    rep.compare("loss", "oracle", b["loss"], cr.loss_of(b["sums"], R, 0.1))
    return rep


def test_checker_passes_on_the_float32_oracle(batch):
    S, b = batch
    rep = _measure(b)
    assert not rep.failures, "\n".join(rep.failures)
    # well inside every kappa: the oracle rounds as the kernels do, in another order
    for out, worst in rep.worst.items():
        assert worst <= cr.KAPPA[out], (out, worst)


@pytest.mark.parametrize("tooth", cr.TEETH)
def test_every_tooth_fails_on_the_oracle(batch, tooth):
    _, b = batch
    rep = _measure(b)
    t = rep.teeth.get(tooth)
    assert t is not None, "the data has no element %s changes" % tooth
    assert t["exceeds"], "%s stays within the bound everywhere" % tooth
    assert t["ratio"] > 1.0, "the oracle passes the reference changed by %s (%.3g)" % (tooth, t["ratio"])
    assert not rep.problems(cr.TEETH)


def _bump(x, i, rel=1e-3):
    x = x.clone()
    flat = x.view(-1)
    flat[i] = flat[i] * (1 + rel) if flat[i] != 0 else 1e-30
    return x


@pytest.mark.parametrize("what", ["colour", "alpha", "d_logits", "w", "d_sigma", "d_t", "depth", "d_colour",
                                  "sums", "loss"])
def test_checker_fails_on_one_wrong_element(batch, what):
    S, b = batch
    b = dict(b)
    x = b[what]
    if what == "depth":
        x = x.clone()
        ray = int(((b["t"] != x[:, None]).all(1) == False).nonzero()[0, 0])     # noqa: E712
        x[ray] = b["t"][ray, 0] if x[ray] != b["t"][ray, 0] else b["t"][ray, -1] + 1.0
        b[what] = x
    else:
        b[what] = _bump(x, int(x.abs().reshape(-1).argmax()))
    rep = _measure(b, teeth=False)
    out = dict(w="weights", sums="loss_sums").get(what, what)
    assert any(f.startswith(out + " ") for f in rep.failures), rep.failures


def test_depth_of_one_sample_is_the_last_t():
    logits, t, _ = cr.make_rays(5, 1, 3)
    fwd = cr.composite_forward(logits, t)
    assert bool(cr.depth_candidates(fwd)[:, 0].all())
