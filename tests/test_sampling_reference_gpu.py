"""The ray generation and sampling kernels against float64 with error budgets (tests/sampling_reference.py).

Every launch goes straight through the C ABI with its outputs filled with NaN, so an element a kernel
leaves unwritten fails.  K1 runs on a camera rig, on cameras built so that rays have exactly zero x / y
direction components, start on a slab plane, start inside the box or see the box behind them, and on
an explicit point list; K2a / K2b / K2ab on a large near/far table with ray ids at its end; K2c on probe
lengths from 3 to 256 over nine density regimes; K2d on the table and per-batch-row forms with
permuted and repeated ray ids.  The deliberately changed references (teeth) must fail.  The sampling
kernels do not depend on the arithmetic mode, so everything but the fused coarse-pass test runs
unchanged under ``--precision bf16x6``."""

import ctypes
import json

import numpy as np
import pytest
import torch

from fourier_feature_nets_amd import ops
from fourier_feature_nets_amd._lib import FfnError, c_i, c_i64
from oracle import ffn_oracle as orc
from tests import sampling_reference as sr
from tests.helpers import look_at_camera

pytestmark = pytest.mark.gpu

PROBES = [3, 4, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129, 191, 192, 193, 255, 256]
RAYS = [1, 3, 4, 5, 257]
MANY_RAYS = [16389, 65541]       # past 4096 workgroups x 4 waves: a wave takes a second ray
MERGES = [(2, 2), (3, 2), (3, 3), (16, 8), (64, 64), (65, 33), (128, 64), (130, 65), (255, 128), (256, 128),
          (256, 2), (256, 256)]
SAMPLES = [1, 2, 3, 63, 64, 65, 255, 256, 1024, 1025]
ANNEALS = [None, 0.2, 0.73, 1.0]
U_MODES = ["linspace", "rand", "entries", "top"]
TABLE = (1 << 21) + 3            # rays in the near/far table of the K2 tests


def dev():
    return torch.device("cuda:0")


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev())


def _report(rep, what, **kw):
    teeth = {k: (round(v["ratio"], 3), v["out"]) for k, v in rep.teeth.items()}
    print("sampling reference", json.dumps(dict(what=what, worst=rep.worst, teeth=teeth, **kw)))


def _f32(x):
    return None if x is None else float(np.float32(x))


# ----------------------------------------------------------------------------------- K1
def _launch_raygen(unproj, cam, W, H, lo, hi, points=None):
    C = unproj.shape[0]
    total = C * W * H
    starts, dirs, nf = _nan(total, 3), _nan(total, 3), _nan(2, total)
    valid = torch.full((total,), 7, dtype=torch.uint8, device=dev())
    ops._call("ffn_raygen_nearfar", ops._dev(unproj), ops._dev(cam), ops._dev(points), c_i(C), c_i(W), c_i(H),
              ops._host3(lo), ops._host3(hi), ops._dev(starts), ops._dev(dirs), ops._dev(nf),
              ops._dev(valid, torch.uint8))
    torch.cuda.synchronize()
    assert bool((valid <= 1).all()), "valid holds something other than 0 / 1"
    return starts.cpu(), dirs.cpu(), nf.cpu(), valid.cpu()


def _rig(n_cam, width, height):
    rng = np.random.RandomState(0)
    unproj, cam = [], []
    for c in range(n_cam):
        ang = 2 * np.pi * c / n_cam + 0.1
        eye = [4 * np.cos(ang), 0.6 + rng.rand(), 4 * np.sin(ang)]
        k, e = look_at_camera(eye, width, height)
        unproj.append(orc.unprojection(k, e))
        cam.append(e[:3, 3])
    return torch.from_numpy(np.stack(unproj).astype(np.float32)), torch.from_numpy(np.stack(cam).astype(np.float32))


def _axis_cameras(eyes, width, height):
    """Cameras looking down -z whose unprojection is written out: world = eye + (a (x - cx), a (y - cy), -1)
    with a = 2^-7, so the ray through (cx, cy) has exactly zero x and y components."""
    a, cx, cy = 2.0 ** -7, width // 2, height // 2
    unproj, cam = [], []
    for e in eyes:
        m = np.array([[a, 0, -a * cx, e[0]], [0, a, -a * cy, e[1]], [0, 0, -1, e[2]], [0, 0, 0, 1]], np.float32)
        unproj.append(m)
        cam.append(np.asarray(e, np.float32))
    return torch.from_numpy(np.stack(unproj)), torch.from_numpy(np.stack(cam))


def _k1_case(rep, key, unproj, cam, W, H, lo, hi, points=None, teeth=True):
    out = _launch_raygen(unproj.to(dev()).contiguous(), cam.to(dev()).contiguous(), W, H, lo, hi,
                         None if points is None else points.to(dev()).contiguous())
    sr.check_raygen(rep, key, unproj, cam, W, H, lo, hi, points, *out, teeth=teeth)
    return out


def test_raygen_against_float64():
    rep = sr.new_report()
    box = ([-1.0] * 3, [1.0] * 3)
    unproj, cam = _rig(8, 400, 400)
    _, _, nf, valid = _k1_case(rep, "rig 8x400x400", unproj, cam, 400, 400, *box)
    assert 0.3 < float(valid.float().mean()) < 0.95
    # zero x / y components (eye on the z axis), rays starting on the lo / hi planes of x and y (0 / 0 in
    # the slab test), a camera inside the box
    eyes = [(0.0, 0.0, 4.0), (-1.0, 0.0, 4.0), (1.0, 0.0, 4.0), (0.0, 1.0, 4.0), (0.05, 0.02, 0.03)]
    unproj, cam = _axis_cameras(eyes, 64, 64)
    starts, dirs, nf, valid = _k1_case(rep, "axis cameras", unproj, cam, 64, 64, *box)
    centre = 32 * 64 + 32
    assert float(dirs[centre, 0]) == 0.0 and float(dirs[centre, 1]) == 0.0
    assert bool(torch.isnan(nf[0, 2 * 4096 + centre])), "a ray on the hi x plane with dx = 0 gives a NaN near"
    assert int(valid[4 * 4096 + centre]) == 1 and float(nf[0, 4 * 4096 + centre]) == sr.NEAR_MIN
    # the box behind the camera: near < far < 0.1, valid with near clamped past far
    unproj, cam = _axis_cameras([(0.0, 0.0, 4.0)], 64, 64)
    _, _, nf, valid = _k1_case(rep, "box behind", unproj, cam, 64, 64, [-1.0, -1.0, 5.0], [1.0, 1.0, 7.0])
    assert int(valid[centre]) == 1 and float(nf[1, centre]) < 0
    # the explicit point list (CameraInfo.raycast): a box of +-1 and the raycast's +-1e30
    g = torch.Generator().manual_seed(5)
    pts = (torch.rand(1000, 2, generator=g) * torch.tensor([400.0, 400.0])).float()
    unproj, cam = _rig(2, 400, 400)
    _k1_case(rep, "points", unproj, cam, 1000, 1, *box, points=pts)
    _k1_case(rep, "points raycast box", unproj[:1], cam[:1], 1000, 1, [-1e30] * 3, [1e30] * 3, points=pts,
             teeth=False)
    _report(rep, "K1")
    problems = rep.problems(sr.K1_TEETH)
    assert not problems, "\n".join(problems)


# ----------------------------------------------------------------------------------- K2a / K2b
@pytest.fixture(scope="module")
def table():
    """near/far (2, TABLE), starts, directions (TABLE, 3) on the GPU and their CPU copies."""
    g = torch.Generator().manual_seed(11)
    near = (0.1 + 2.0 * torch.rand(TABLE, generator=g)).float()
    far = (near.double() + 0.25 + 4.0 * torch.rand(TABLE, generator=g, dtype=torch.float64)).float()
    starts = (torch.rand(TABLE, 3, generator=g) * 4 - 2).float()
    dirs = torch.nn.functional.normalize(torch.randn(TABLE, 3, generator=g, dtype=torch.float64), dim=1).float()
    cpu = dict(near_far=torch.stack([near, far]).contiguous(), starts=starts.contiguous(), dirs=dirs.contiguous())
    return dict(cpu=cpu, gpu={k: v.to(dev()) for k, v in cpu.items()})


def _ray_ids(R, seed, total=TABLE):
    """R ids: the last ones of the table, repeats, random ones, in a shuffled order."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, total, (R,), generator=g)
    tail = torch.arange(total - 1, total - 1 - min(R, 40), -1)
    ids[:tail.numel()] = tail
    if R > 60:
        ids[40:50] = ids[50:60]
    return ids[torch.randperm(R, generator=g)].contiguous()


def _k2_case(rep, table, R, S, anneal, stratified, seed, teeth):
    key = "R=%d S=%d anneal=%s stratified=%s" % (R, S, anneal, stratified)
    cpu, gpu = table["cpu"], table["gpu"]
    idx = _ray_ids(R, seed)
    assert 0 <= int(idx.min()) and int(idx.max()) < TABLE
    idx_d = idx.to(dev())
    unit = torch.linspace(0, 1, S)
    unit_d = unit.to(dev())
    g = torch.Generator().manual_seed(seed + 1)
    noise = torch.rand(R, S, generator=g) if stratified else None
    noise_d = None if noise is None else noise.to(dev())
    a = -1.0 if anneal is None else anneal
    stride = S + 3
    t_s = _nan(R, stride)
    ops._call("ffn_sample_t", ops._dev(gpu["near_far"]), c_i64(TABLE), ops._dev(idx_d, torch.int64), c_i(R), c_i(S),
              ops._dev(unit_d), ops._dev(noise_d), ops.c_f(a), ops._dev(t_s), c_i(stride))
    t = t_s[:, :S].contiguous()
    pos, views = _nan(R, S, 3), _nan(R, S, 3)
    ops._call("ffn_materialise_samples", ops._dev(gpu["starts"]), ops._dev(gpu["dirs"]), ops._dev(idx_d, torch.int64),
              ops._dev(t), c_i(R), c_i(S), ops._dev(pos), ops._dev(views))
    t1, pos1, views1 = _nan(R, S), _nan(R, S, 3), _nan(R, S, 3)
    ops._call("ffn_sample_materialise", ops._dev(gpu["near_far"]), c_i64(TABLE), ops._dev(gpu["starts"]),
              ops._dev(gpu["dirs"]), ops._dev(idx_d, torch.int64), c_i(R), c_i(S), ops._dev(unit_d), ops._dev(noise_d),
              ops.c_f(a), ops._dev(t1), ops._dev(pos1), ops._dev(views1))
    torch.cuda.synchronize()
    assert bool(torch.isnan(t_s[:, S:]).all()), "%s: K2a wrote past count in a strided row" % key
    assert torch.equal(t1, t), "%s: the one-launch t differs from K2a's" % key
    assert torch.equal(pos1, pos), "%s: the one-launch positions differ from K2b's" % key
    assert torch.equal(views1, views), "%s: the one-launch views differ from K2b's" % key
    t, pos, views = t.cpu(), pos.cpu(), views.cpu()
    near, far = cpu["near_far"][0][idx], cpu["near_far"][1][idx]
    sr.check_sample_t(rep, key, near, far, unit, noise, anneal, t, teeth=teeth)
    sr.check_positions(rep, key, cpu["starts"][idx], cpu["dirs"][idx], t, pos, views)


@pytest.mark.parametrize("S", SAMPLES)
def test_sample_t_and_materialise_against_float64(table, S):
    rep = sr.new_report()
    for i, anneal in enumerate(ANNEALS):
        for stratified in (False, True):
            for R in RAYS:
                if R != 257 and anneal not in (None, 0.73):
                    continue
                _k2_case(rep, table, R, S, _f32(anneal), stratified, 100 * S + 10 * i + R, teeth=R == 257)
    _report(rep, "K2", S=S)
    problems = rep.problems(sr.K2_TEETH)
    assert not problems, "\n".join(problems)


# ----------------------------------------------------------------------------------- K2c
def _launch_cdf(t, opacity, logits):
    R, n = t.shape
    t_d, op_d = t.to(dev()), opacity.to(dev())        # (held until the launch has run)
    cdf = _nan(R, n - 1)
    ops._call("ffn_cdf_build_logits" if logits else "ffn_cdf_build", ops._dev(t_d), ops._dev(op_d), c_i64(R), c_i(n),
              ops._dev(cdf))
    torch.cuda.synchronize()
    return cdf


def _cdf_case(rep, R, n, seed, teeth):
    t, logits, sigma = sr.make_probe(R, n, seed)
    c_plain = _launch_cdf(t, sigma, False)
    c_logits = _launch_cdf(t, logits, True)
    torch.cuda.synchronize()
    key = "R=%d n=%d" % (R, n)
    sr.check_cdf(rep, key + " sigma", t, sigma, c_plain.cpu(), logits=False, teeth=teeth)
    sr.check_cdf(rep, key + " logits", t, logits, c_logits.cpu(), logits=True, teeth=teeth)
    return t, logits, c_logits.cpu()


@pytest.mark.parametrize("n", PROBES)
def test_cdf_build_against_float64(n):
    rep = sr.new_report()
    for R in RAYS:
        _cdf_case(rep, R, n, 1000 * n + R, teeth=R == 257)
    _report(rep, "K2c", n=n)
    problems = rep.problems(sr.cdf_teeth(n))
    assert not problems, "\n".join(problems)


@pytest.mark.parametrize("n", [64, 65, 256])
@pytest.mark.parametrize("R", MANY_RAYS)
def test_cdf_build_several_rays_per_wave(R, n):
    rep = sr.new_report()
    _cdf_case(rep, R, n, 7 * n + R, teeth=False)
    _report(rep, "K2c many", n=n, R=R)
    assert not rep.failures, "\n".join(rep.failures)


# ----------------------------------------------------------------------------------- K2d
def _cdf_table(Rt, n_focus, seed):
    """near / far (Rt,) and CDF rows (Rt, n_focus - 1): the kernel's own (K2c on probe points of those
    near / far), the single row [0] for n_focus = 2."""
    if n_focus == 2:
        _, near, far = sr.probe_t(Rt, 3, seed)
        return near, far, torch.zeros(Rt, 1)
    t, logits, _ = sr.make_probe(Rt, n_focus, seed)
    _, near, far = sr.probe_t(Rt, n_focus, seed)
    cdf = _launch_cdf(t, logits, True)
    torch.cuda.synchronize()
    return near, far, cdf.cpu()


def _merge_case(rep, R, S, n_focus, mode, seed, teeth, rows_local):
    Rt = R + 40
    near, far, cdf = _cdf_table(Rt, n_focus, seed)
    g = torch.Generator().manual_seed(seed + 3)
    idx = torch.randint(0, Rt, (R,), generator=g)
    if R > 3:
        idx[1] = idx[0]
    idx = idx.contiguous()
    assert 0 <= int(idx.min()) and int(idx.max()) < Rt
    n_uniform = S - n_focus
    unit_u = torch.linspace(0, 1, n_uniform) if n_uniform > 0 else torch.zeros(0)
    uniform_in = orc.uniform_t(near[idx], far[idx], n_uniform, torch.rand(R, n_uniform, generator=g), unit_u) \
        if n_uniform > 0 else torch.zeros(R, 0)
    u = sr.make_u(cdf[idx], n_focus, seed + 4, mode)
    unit = torch.linspace(0, 1, n_focus)
    t_io = torch.cat([uniform_in, torch.full((R, n_focus), float("nan"))], 1).to(dev()).contiguous()
    near_far = torch.stack([near, far]).to(dev()).contiguous()
    rows = (cdf[idx] if rows_local else cdf).to(dev()).contiguous()
    idx_d, u_d, unit_d = idx.to(dev()), u.to(dev()), unit.to(dev())      # (held until the launch has run)
    ops._call("ffn_focus_sample_merge_rows" if rows_local else "ffn_focus_sample_merge", ops._dev(near_far),
              c_i64(Rt), ops._dev(rows), ops._dev(idx_d, torch.int64), ops._dev(u_d), ops._dev(unit_d), c_i(R), c_i(S),
              c_i(n_focus), ops._dev(t_io))
    torch.cuda.synchronize()
    key = "R=%d S=%d n_focus=%d u=%s %s" % (R, S, n_focus, mode, "rows" if rows_local else "table")
    sr.check_merge(rep, key, near[idx], far[idx], cdf[idx], u, unit, uniform_in, t_io.cpu(), teeth=teeth)


@pytest.mark.parametrize("S,n_focus", MERGES)
def test_focus_merge_against_float64(S, n_focus):
    rep = sr.new_report()
    for R in RAYS:
        for m, mode in enumerate(U_MODES):
            if R not in (5, 257) and mode != "entries":
                continue
            for rows_local in (False, True):
                _merge_case(rep, R, S, n_focus, mode, 1000 * S + 10 * n_focus + R + m, R == 257, rows_local)
    _report(rep, "K2d", S=S, n_focus=n_focus)
    problems = rep.problems(sr.merge_teeth(n_focus))
    assert not problems, "\n".join(problems)


@pytest.mark.parametrize("S,n_focus", [(128, 64), (256, 128)])
@pytest.mark.parametrize("R", MANY_RAYS)
def test_focus_merge_several_rays_per_wave(R, S, n_focus):
    rep = sr.new_report()
    for rows_local in (False, True):
        _merge_case(rep, R, S, n_focus, "entries", R + S, False, rows_local)
    _report(rep, "K2d many", S=S, n_focus=n_focus, R=R)
    assert not rep.failures, "\n".join(rep.failures)


# ----------------------------------------------------------------------------------- fused focus
def _coarse_models():
    from tests.helpers import GOLDEN
    from tests.test_kernels_gpu import _load_fourier, _load_nerf
    from tests.test_pipeline_gpu import _small_model
    g = np.load(GOLDEN + "/models.npz", allow_pickle=False)
    tr = np.load(GOLDEN + "/training.npz", allow_pickle=False)
    return [("tiny", _small_model(tr)), ("nerf_small", _load_nerf(g, "nerf_small", [2], False)[0]),
            ("gaussian512", _load_fourier(g, "gaussian512")[0])]


def _five_launches(model, table, idx, S, n_focus, unit, u, t_io):
    """sample_t probe, materialise, forward, cdf_build_logits, focus_sample_merge(rows_local=True)."""
    gpu = table["gpu"]
    t_probe = ops.sample_t(gpu["near_far"], idx, n_focus, unit, None, None)
    pos, views = ops.materialise_samples(gpu["starts"], gpu["dirs"], idx, t_probe, want_views=model.use_view)
    with torch.no_grad():
        logits = model(pos.reshape(-1, 3), views.reshape(-1, 3)) if model.use_view else model(pos.reshape(-1, 3))
    cdf = ops.cdf_build_logits(t_probe, logits.contiguous())
    ops.focus_sample_merge(gpu["near_far"], cdf, idx, u, unit, t_io, n_focus, rows_local=True)
    return t_probe, logits, cdf


@pytest.mark.exact_only(reason="the fused coarse-pass kernel is exact-f32 only")
def test_fused_focus_equals_the_five_launches(table):
    rep = sr.new_report()
    gpu = table["gpu"]
    for name, model in _coarse_models():
        prog = model.program()
        for n_focus in (3, 4, 31, 32, 33, 63, 64):
            for S in sorted({n_focus, n_focus + 1, 2 * n_focus, 256}):
                for R in (1, 2, 3, 5, 777, 5000):
                    seed = 10 * S + n_focus + R
                    idx = _ray_ids(R, seed).to(dev())
                    n_uniform = S - n_focus
                    g = torch.Generator(device=dev()).manual_seed(seed)
                    t0 = _nan(R, S)
                    if n_uniform > 0:
                        noise = torch.rand(R, n_uniform, generator=g, device=dev())
                        ops.sample_t(gpu["near_far"], idx, n_uniform, torch.linspace(0, 1, n_uniform).to(dev()), noise,
                                     None, out=t0)
                    u = torch.rand(R, n_focus, generator=g, device=dev())
                    unit = torch.linspace(0, 1, n_focus).to(dev())
                    five = t0.clone()
                    t_probe, logits, cdf = _five_launches(model, table, idx, S, n_focus, unit, u, five)
                    fused = t0.clone()
                    prog.focus_sample(gpu["starts"], gpu["dirs"], gpu["near_far"], idx, S, n_focus, unit, u, fused)
                    torch.cuda.synchronize()
                    key = "%s R=%d S=%d n_focus=%d" % (name, R, S, n_focus)
                    assert torch.equal(fused, five), key + ": the fused kernel differs from the five launches"
                    if R == 777 and S == 2 * n_focus:
                        # the live path's own CDF and merge against the references
                        ic = idx.cpu()
                        sr.check_cdf(rep, key, t_probe.cpu(), logits.cpu(), cdf.cpu(), logits=True, teeth=False)
                        nf = table["cpu"]["near_far"]
                        sr.check_merge(rep, key, nf[0][ic], nf[1][ic], cdf.cpu(), u.cpu(), unit.cpu(),
                                       t0[:, :n_uniform].cpu(), five.cpu(), teeth=False)
    _report(rep, "fused")
    assert not rep.failures, "\n".join(rep.failures)


# ----------------------------------------------------------------------------------- refusals
def _refused(match, fn, *outs):
    with pytest.raises(FfnError, match=match):
        fn()
    torch.cuda.synchronize()
    for o in outs:
        assert bool(torch.isnan(o).all()), "%s: the refused call wrote its output" % match


def test_out_of_range_shapes_are_refused_before_any_launch(table):
    gpu = table["gpu"]
    for n in (2, 257):
        t = torch.zeros((4, n), dtype=torch.float32, device=dev())
        cdf = _nan(4, n - 1)
        _refused("probe length", lambda: ops._call("ffn_cdf_build", ops._dev(t), ops._dev(t), c_i64(4), c_i(n),
                                                   ops._dev(cdf)), cdf)
        logits = torch.zeros((4 * n, 4), dtype=torch.float32, device=dev())
        _refused("probe length", lambda: ops._call("ffn_cdf_build_logits", ops._dev(t), ops._dev(logits), c_i64(4),
                                                   c_i(n), ops._dev(cdf)), cdf)
    idx = torch.arange(4, dtype=torch.int64, device=dev())
    for S, n_focus in ((257, 128), (16, 1), (16, 17)):
        t_io = _nan(4, S)
        cdf = torch.zeros((4, max(n_focus - 1, 1)), dtype=torch.float32, device=dev())
        u = torch.zeros((4, n_focus), dtype=torch.float32, device=dev())
        unit = torch.linspace(0, 1, n_focus).to(dev())
        for name in ("ffn_focus_sample_merge", "ffn_focus_sample_merge_rows"):
            _refused("n_focus <= S <= 256", lambda: ops._call(
                name, ops._dev(gpu["near_far"]), c_i64(TABLE), ops._dev(cdf), ops._dev(idx, torch.int64), ops._dev(u),
                ops._dev(unit), c_i(4), c_i(S), c_i(n_focus), ops._dev(t_io)), t_io)


@pytest.mark.exact_only(reason="builds a coarse model's exact-f32 program")
def test_fused_focus_shapes_are_refused_before_any_launch(table):
    gpu = table["gpu"]
    model = _coarse_models()[0][1]
    prog = model.program()
    idx = torch.arange(4, dtype=torch.int64, device=dev())
    for n_focus in (2, 65):
        t_io = _nan(4, 128)
        u = torch.zeros((4, n_focus), dtype=torch.float32, device=dev())
        unit = torch.linspace(0, 1, n_focus).to(dev())
        _refused("3 <= n_focus <= 64", lambda: ops._call(
            "ffn_focus_fused", ctypes.byref(prog.fwd), ops._dev(prog.packed_fwd), ops._dev(prog.bias_buf),
            ops._dev(gpu["starts"]), ops._dev(gpu["dirs"]), ops._dev(gpu["near_far"]), c_i64(TABLE),
            ops._dev(idx, torch.int64), c_i(4), c_i(128), c_i(n_focus), ops._dev(unit), ops._dev(u), ops._dev(t_io)),
            t_io)
