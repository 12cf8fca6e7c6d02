"""The float64 ray-generation / sampling checker (tests/sampling_reference.py) on the float32 CPU oracle,
no GPU needed: ``orc.raycast`` / ``near_far`` / ``uniform_t`` / ``determine_cdf`` / ``focus_t`` and the
sort.  The checker must pass on them, every deliberately changed reference must fail on them, and one
wrong element must fail."""

import numpy as np
import pytest
import torch

from oracle import ffn_oracle as orc
from tests import sampling_reference as sr
from tests.helpers import look_at_camera

R = 257
PROBES = [3, 4, 64, 65, 130, 256]


def _raygen(box_lo, box_hi, eyes, W=48, H=40):
    """The oracle's K1 outputs for cameras at ``eyes`` looking at the origin, with the kernel's inputs."""
    unproj, cam, outs = [], [], []
    pts = orc.pixel_grid(W, H)
    for eye in eyes:
        k, e = look_at_camera(eye, W, H)
        unproj.append(orc.unprojection(k, e))
        cam.append(e[:3, 3])
        s, d = orc.raycast(k, e, pts)
        nf, ok = orc.near_far(s, d, np.float32(box_lo)[None], np.float32(box_hi)[None])
        outs.append((s, d, nf, ok))
    cat = [torch.from_numpy(np.concatenate([o[i] for o in outs], -1 if i == 2 else 0).astype(np.float32 if i < 3 else np.uint8))
           for i in range(4)]
    return (torch.from_numpy(np.stack(unproj).astype(np.float32)), torch.from_numpy(np.stack(cam).astype(np.float32)),
            W, H) + tuple(cat)


RIGS = dict(outside=([-1.0] * 3, [1.0] * 3, [(3.0, 0.7, 2.5), (-2.0, 1.1, -3.0)]),
            inside=([-1.0] * 3, [1.0] * 3, [(0.3, 0.2, 0.1)]),
            behind=([-1.0, -1.0, 5.0], [1.0, 1.0, 7.0], [(0.5, 0.3, 4.0)]))


def _check_raygen(rig, teeth=True, **override):
    lo, hi, eyes = RIGS[rig]
    unproj, cam, W, H, starts, dirs, nf, valid = _raygen(lo, hi, eyes)
    outs = dict(starts=starts, dirs=dirs, nf=nf, valid=valid)
    outs.update(override)
    rep = sr.new_report()
    sr.check_raygen(rep, "oracle " + rig, unproj, cam, W, H, lo, hi, None, outs["starts"], outs["dirs"], outs["nf"],
                    outs["valid"], teeth=teeth)
    return rep, outs


def test_raygen_checker_passes_on_the_oracle():
    for rig in RIGS:
        rep, _ = _check_raygen(rig)
        assert not rep.failures, "\n".join(rep.failures)
        for out, worst in rep.worst.items():
            assert worst <= sr.KAPPA[out], (rig, out, worst)


@pytest.mark.parametrize("tooth,rig", [("pixel_centre", "outside"), ("near_unclamped", "inside"),
                                       ("clamp_before_test", "behind")])
def test_raygen_teeth_fail_on_the_oracle(tooth, rig):
    rep, _ = _check_raygen(rig)
    t = rep.teeth.get(tooth)
    assert t is not None and t["exceeds"] and t["ratio"] > 1.0, (tooth, t)


def test_raygen_checker_fails_on_one_wrong_element():
    rep, outs = _check_raygen("outside", teeth=False)
    d = outs["dirs"].clone()
    d[5, 1] = d[5, 1] * (1 + 1e-5)
    assert any(f.startswith("dirs ") for f in _check_raygen("outside", teeth=False, dirs=d)[0].failures)
    nf = outs["nf"].clone()
    i = int(outs["valid"].nonzero()[0, 0])
    nf[1, i] = nf[1, i] * (1 + 1e-5)
    assert any(f.startswith("near_far ") for f in _check_raygen("outside", teeth=False, nf=nf)[0].failures)
    v = outs["valid"].clone()
    v[i] = 0
    assert any(f.startswith("valid ") for f in _check_raygen("outside", teeth=False, valid=v)[0].failures)
    s = outs["starts"].clone()
    s[3, 0] = float(np.nextafter(np.float32(s[3, 0]), np.float32(np.inf)))
    assert any(f.startswith("starts ") for f in _check_raygen("outside", teeth=False, starts=s)[0].failures)


# ----------------------------------------------------------------------------------- K2a / K2b
def _rays(n, seed):
    g = torch.Generator().manual_seed(seed)
    near = (0.1 + 2.0 * torch.rand(n, generator=g)).float()
    far = (near.double() + 0.25 + 4.0 * torch.rand(n, generator=g, dtype=torch.float64)).float()
    starts = (torch.rand(n, 3, generator=g) * 4 - 2).float()
    dirs = torch.nn.functional.normalize(torch.randn(n, 3, generator=g, dtype=torch.float64), dim=1).float()
    return near, far, starts, dirs, torch.rand(n, 65, generator=g)


@pytest.mark.parametrize("anneal", [None, float(np.float32(0.73))])
def test_sample_t_checker_on_the_oracle(anneal):
    near, far, starts, dirs, noise = _rays(R, 3)
    unit = torch.linspace(0, 1, 65)
    rep = sr.new_report()
    for nz in (None, noise):
        t = sr.uniform_t32(near, far, unit, nz, anneal)
        sr.check_sample_t(rep, "oracle", near, far, unit, nz, anneal, t)
        pos = sr.positions32(starts, dirs, t)
        sr.check_positions(rep, "oracle", starts, dirs, t, pos, dirs[:, None, :].expand(-1, 65, 3).contiguous())
    assert not rep.failures, "\n".join(rep.failures)
    teeth = ("stratified_scale", "anneal_about_near") if anneal is not None else ("stratified_scale",)
    assert not rep.problems(teeth), rep.problems(teeth)
    bad = t.clone()
    bad[7, 9] = float(np.nextafter(np.float32(bad[7, 9]), np.float32(np.inf)))
    rep = sr.new_report()
    sr.check_sample_t(rep, "oracle", near, far, unit, noise, anneal, bad, teeth=False)
    assert any(f.startswith("t ") for f in rep.failures)


# ----------------------------------------------------------------------------------- K2c
@pytest.fixture(scope="module", params=PROBES)
def probe(request):
    n = request.param
    t, logits, sigma = sr.make_probe(R, n, 5 * n)
    return n, t, logits, sigma, orc.determine_cdf(t, sigma)


def test_cdf_checker_passes_on_the_oracle(probe):
    n, t, logits, sigma, cdf = probe
    rep = sr.new_report()
    # the oracle's cumsum is sequential: its sum depth is n
    sr.check_cdf(rep, "oracle", t, sigma, cdf, sum_depth=n)
    sr.check_cdf(rep, "oracle logits", t, logits, cdf, logits=True, sum_depth=n)
    assert not rep.failures, "\n".join(rep.failures)
    problems = rep.problems(sr.cdf_teeth(n))
    assert not problems, "\n".join(problems)


def test_cdf_checker_fails_on_one_wrong_element(probe):
    n, t, logits, sigma, cdf = probe
    # the element with the tightest budget, moved by 4 of its bounds
    ref = sr.cdf64(t, sigma, sum_depth=n)
    rel = torch.where(ref.v > 0, ref.b * sr.U / ref.v.clamp_min(1e-300), float("inf"))
    i = int(rel.argmin())
    bad = cdf.clone()
    bad.view(-1)[i] = float(ref.v.view(-1)[i] * (1 + 4 * sr.KAPPA["cdf"] * float(rel.view(-1)[i])))
    rep = sr.new_report()
    sr.check_cdf(rep, "oracle", t, sigma, bad, sum_depth=n, teeth=False)
    assert any(f.startswith("cdf ") for f in rep.failures)


# ----------------------------------------------------------------------------------- K2d
@pytest.mark.parametrize("S,n_focus", [(16, 8), (130, 65), (256, 128), (256, 2)])
@pytest.mark.parametrize("mode", ["linspace", "entries", "top"])
def test_merge_checker_on_the_oracle(S, n_focus, mode):
    t, logits, sigma = sr.make_probe(R, max(n_focus, 3), n_focus)
    _, near, far = sr.probe_t(R, max(n_focus, 3), n_focus)
    cdf = orc.determine_cdf(t, sigma) if n_focus > 2 else torch.zeros(R, 1)
    u = sr.make_u(cdf, n_focus, S, mode)
    unit = torch.linspace(0, 1, n_focus)
    n_uniform = S - n_focus
    uniform = orc.uniform_t(near, far, n_uniform, torch.rand(R, n_uniform), torch.linspace(0, 1, n_uniform))
    row = torch.cat([uniform, orc.focus_t(near, far, cdf, u, unit)], -1).sort(-1).values
    rep = sr.new_report()
    sr.check_merge(rep, "oracle", near, far, cdf, u, unit, uniform, row)
    assert not rep.failures, "\n".join(rep.failures)
    required = [x for x in sr.merge_teeth(n_focus) if x != "right_false" or mode == "entries"]
    problems = rep.problems(required)
    assert not problems, "\n".join(problems)
    bad = row.clone()
    bad[3, S // 2] = float(np.nextafter(np.float32(bad[3, S // 2]), np.float32(0)))
    rep = sr.new_report()
    sr.check_merge(rep, "oracle", near, far, cdf, u, unit, uniform, bad, teeth=False)
    assert any(f.startswith("row ") for f in rep.failures)
