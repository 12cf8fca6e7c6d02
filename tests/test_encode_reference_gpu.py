"""K3 ``ffn_fourier_encode`` against float64 at every branch of its launch plan, and the u8 pixel
writers (K8 ``ffn_to_image`` and the fused render kernel's image output) byte for byte
(references, budget and the shape list: tests/encode_reference.py).

K3 writes into a NaN-filled slice of a larger buffer whose other floats hold a guard value: an
element the kernel leaves unwritten shows up as NaN, a store outside the rows as a changed guard.
A refused call must leave both untouched."""

import json
import math

import numpy as np
import pytest
import torch

from fourier_feature_nets_amd import ops
from fourier_feature_nets_amd._lib import FfnError, c_f, c_i, c_i64
from tests import encode_reference as er

pytestmark = pytest.mark.gpu

GUARD = 12345.0
FRONT = 4               # guard floats in front of the rows (keeps them 16-byte aligned)
BACK = 1024             # guard floats behind them
FUSED_KERNELS_ARE_EXACT_F32 = "the fused kernel is exact f32"


def dev():
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------ K3
def _inputs(freq, n, seed, block_diagonal=False, amplitudes=True):
    """x uniform in [-1, 1]^3 with rows of 0, -0.0 and +-1, b = randn * 2 (or NeRF's block-diagonal
    octaves), a in [0.5, 2] or None: CPU float32."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand(n, 3, generator=gen) * 2 - 1
    special = torch.tensor([[0.0, 0.0, 0.0], [-0.0, -0.0, -0.0], [1.0, 1.0, 1.0], [-1.0, -1.0, -1.0],
                            [1.0, -1.0, 0.0]])
    if n >= 2 * len(special):
        x[1:2 * len(special):2] = special
    if freq == 0:
        return x, None, None
    b = er.block_diagonal_b(freq) if block_diagonal else torch.randn(3, freq, generator=gen) * 2
    a = torch.rand(freq, generator=gen) * 1.5 + 0.5 if amplitudes else None
    return x, b, a


def _ptr_at(buf, offset):
    """Device pointer of ``buf[offset]`` (also where the rows are empty or must be misaligned)."""
    p = ops._DevPtr(buf.data_ptr() + buf.element_size() * offset)
    p.device = buf.device
    return p


def _encode_raw(x, b, a, freq, scale, inc, n=None, front=FRONT):
    """The entry point itself, writing (n, width) rows at float ``front`` of a guard-filled
    buffer: (rows, whole buffer).  Tensors are device tensors or None."""
    n = int(x.shape[0]) if n is None else n
    width = 2 * freq + (3 if (inc or freq == 0) else 0)
    rows = n * width
    buf = torch.full((front + rows + BACK,), GUARD, dtype=torch.float32, device=dev())
    buf[front:front + rows] = float("nan")
    ops._call("ffn_fourier_encode", ops._dev(x), c_i64(n), ops._dev(b), ops._dev(a), c_i(freq), c_f(scale),
              c_i(1 if inc else 0), _ptr_at(buf, front))
    torch.cuda.synchronize()
    return buf[front:front + rows].view(n, width), buf


def _guards_intact(buf, front, rows):
    return bool((buf[:front] == GUARD).all()) and bool((buf[front + rows:] == GUARD).all())


def _check(key, x, b, a, scale, inc, worst):
    """One K3 call on CPU float32 inputs: guards, no NaN, pass-through bits, the budget.  Returns
    the device rows."""
    freq = 0 if b is None else int(b.shape[1])
    xd = x.to(dev())
    bd = None if b is None else b.contiguous().to(dev())
    ad = None if a is None else a.to(dev())
    got, buf = _encode_raw(xd, bd, ad, freq, scale, inc)
    assert _guards_intact(buf, FRONT, got.numel()), key + ": a float outside the rows was written"
    assert not bool(torch.isnan(got).any()), key + ": an element was left unwritten"
    if inc or freq == 0:                    # a copy has no rounding: the bits of x, -0.0 included
        assert torch.equal(got[:, 2 * freq:].view(torch.int32), xd.view(torch.int32)), key + ": pass-through bits"
    ref, terms = er.encode_features(xd.double(), None if bd is None else bd.double(),
                                    None if ad is None else ad.double(), scale, inc)
    ratio, failures = er.check_features(key, got, ref, terms)
    worst.append((ratio, key))
    assert not failures, "\n".join(failures)
    return got


def _report(worst, what):
    ratio, key = max(worst) if worst else (0.0, "-")
    print("K3 reference", json.dumps(dict(cases=what, worst_ratio=ratio, at=key, kappa=er.KAPPA)))


@pytest.mark.parametrize("inc", [False, True])
def test_every_frequency_count_at_a_ragged_row_count(inc):
    """F = 0 .. 1025 (one lane per sample, idle threads, odd F, slots repeating pair 0, a thread
    looping over slots, every rule for the rows per block) at two groups and three rows."""
    worst = []
    for freq in er.FREQS:
        n = er.ragged_rows(freq, inc)
        diag = inc and freq % 3 == 0 and freq > 0
        x, b, a = _inputs(freq, n, 100 * freq + inc, block_diagonal=diag, amplitudes=not (inc and freq % 2 == 0))
        scale = 1.0 if diag else math.pi
        _check("F=%d inc=%d n=%d" % (freq, inc, n), x, b, a, scale, inc, worst)
    _report(worst, "frequency counts, include_input=%d" % inc)


@pytest.mark.parametrize("freq", er.ROW_SWEEP_FREQS)
def test_every_row_count_around_a_group(freq):
    """n = 0 .. 5, group - 1, group, group + 1, 2 group + 3 with odd widths (9, 129, 517): the
    scalar store tail with 1, 2 and 3 floats, a lone ragged group, n = 0 writing nothing."""
    worst = []
    for n in er.row_sweep(freq):
        x, b, a = _inputs(freq, n, 7 * freq + n, block_diagonal=freq == 63)
        scale = 1.0 if freq == 63 else 1.5
        _check("F=%d inc=1 n=%d" % (freq, n), x, b, a, scale, True, worst)
    _report(worst, "row counts at F=%d" % freq)


@pytest.mark.parametrize("freq,inc,n", er.GRID_STRIDE)
def test_more_groups_than_blocks(freq, inc, n):
    """Past 4096 groups a block takes several: its tile is reused behind a barrier."""
    assert er.grid_strides(freq, inc, n) and not er.grid_strides(freq, inc, n - 130)
    worst = []
    x, b, a = _inputs(freq, n, n)
    _check("F=%d inc=%d n=%d" % (freq, inc, n), x, b, a, math.pi, inc, worst)
    _report(worst, "grid stride")


def test_no_amplitudes_means_ones_and_calls_repeat():
    for freq, inc, n in ((7, True, 259), (256, False, 67)):
        x, b, _ = _inputs(freq, n, freq)
        xd, bd = x.to(dev()), b.contiguous().to(dev())
        bare, _ = _encode_raw(xd, bd, None, freq, 1.5, inc)
        ones, _ = _encode_raw(xd, bd, torch.ones(freq, device=dev()), freq, 1.5, inc)
        again, _ = _encode_raw(xd, bd, None, freq, 1.5, inc)
        assert torch.equal(bare.view(torch.int32), ones.view(torch.int32))
        assert torch.equal(bare.view(torch.int32), again.view(torch.int32))
        assert torch.equal(ops.fourier_encode(xd, bd, None, 1.5, inc).view(torch.int32), bare.view(torch.int32))


def test_angles_up_to_the_documented_limit():
    """The scale chosen, in float64, so that the largest |angle| of the batch is about 4500 rad
    (common.h states the polynomial's error for |x| <= 5000): a wrong quadrant or a broken
    reduction is O(1), the budget at these angles a few 1e-3."""
    worst = []
    x, b, a = _inputs(85, 1003, 5)
    top = float((x.double() @ b.double()).abs().max())
    scale = float(np.float32(4500.0 / top))
    largest = scale * top
    print("K3 angles", json.dumps(dict(scale=scale, largest_angle=largest)))
    assert 4000.0 <= largest <= 5000.0
    _check("F=85 large angles", x, b, a, scale, True, worst)
    _report(worst, "large angles")


@pytest.mark.parametrize("name", ["fold256_1", "fold64_2", "positional", "nerf"])
def test_same_bits_as_the_fused_kernels(name):
    """A training forward of 1000 samples in exact f32 leaves the features its first layer read in
    an encoding slab; K3 on the same x, b, a, scale gives the same bits, column by column (both
    run mul, fma, fma, fast_sincos_n, one multiply by the amplitude)."""
    from tests.test_layer_reference_gpu import _inputs as chain_inputs, _model
    model = _model(name)
    prog = model.program()
    n = 1000
    x, views, _ = chain_inputs(model, n)
    saved = torch.full((prog.saved_floats(n),), float("nan"), device=dev())
    prog.forward(x, views, saved, precision="f32")
    acts, _ = prog._split_saved(saved, n)
    assert prog.enc_slot, "the chain has no encoding"
    if name == "nerf":
        assert len(prog.enc_slot) == 2 and any(prog.encodings[e].include_input for e in prog.enc_slot)
    for e, slot in prog.enc_slot.items():
        enc = prog.encodings[e]
        assert enc.num_freq > 0 and enc.num_inputs == 3
        source = (x, views)[e]
        slab = prog.slot_rows(acts, n, slot)[:n]
        k3 = ops.fourier_encode(source.contiguous(), enc.b.to(dev()), enc.a.to(dev()), enc.scale, enc.include_input)
        seen = 0
        for c in range(enc.width):
            nat = enc.natural_index(c)
            if nat < 0:
                continue
            seen += 1
            same = torch.equal(slab[:, c], k3[:, nat])
            assert same, ("%s encoding %d: natural column %d (internal channel %d) differs from the fused "
                          "kernel's in %d of %d rows" % (name, e, nat, c, int((slab[:, c] != k3[:, nat]).sum()), n))
        assert seen == k3.shape[1] == enc.natural_width


# ------------------------------------------------------------------------------------------ K3 limits
def _lds_limit():
    return int(torch.cuda.get_device_properties(0).shared_memory_per_block)


@pytest.mark.parametrize("freq,inc", er.LIMIT_SHAPES)
def test_widest_rows_fit_or_are_refused_by_their_lds_need(freq, inc):
    """Four rows of up to 64 KiB plus the kernel's 1536 B of staged points: where the device's
    per-workgroup LDS limit covers that, the values are within budget; where it does not, the call
    is refused with both figures and writes nothing."""
    plan = er.encode_plan(freq, inc)
    limit = _lds_limit()
    print("K3 LDS", json.dumps(dict(F=freq, include_input=inc, need=plan["lds"], device_limit=limit,
                                    fits=plan["lds"] <= limit)))
    x, b, a = _inputs(freq, 5, freq)
    if plan["lds"] <= limit:
        worst = []
        _check("F=%d inc=%d n=5" % (freq, inc), x, b, a, 0.25, inc, worst)
        _report(worst, "size limit")
        return
    assert er.encode_plan(freq, inc, lds_limit=limit) is None
    xd, bd, ad = x.to(dev()), b.contiguous().to(dev()), a.to(dev())
    _nothing_written(lambda out, buf: ops._call(
        "ffn_fourier_encode", ops._dev(xd), c_i64(5), ops._dev(bd), ops._dev(ad), c_i(freq), c_f(0.25),
        c_i(1 if inc else 0), ops._dev(out)), 5 * plan["width"],
        "needs %d B of LDS, the device allows %d B" % (plan["lds"], limit))


def _nothing_written(call, floats, match, front=FRONT, error=FfnError):
    """``call(out rows, buffer)`` is refused by name and leaves rows and guards as they were."""
    buf = torch.full((front + floats + BACK,), GUARD, dtype=torch.float32, device=dev())
    buf[front:front + floats] = float("nan")
    with pytest.raises(error, match=match):
        call(buf[front:front + floats], buf)
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[front:front + floats]).all()), "%s: the refused call wrote its output" % match
    assert _guards_intact(buf, front, floats), "%s: the refused call wrote outside its output" % match


@pytest.mark.parametrize("freq,inc", er.TOO_WIDE)
def test_too_wide_rows_are_refused_by_name(freq, inc):
    assert er.encode_plan(freq, inc) is None
    x, b, a = _inputs(freq, 5, freq)
    xd, bd, ad = x.to(dev()), b.contiguous().to(dev()), a.to(dev())
    width = 2 * freq + (3 if inc else 0)
    _nothing_written(lambda out, buf: ops._call(
        "ffn_fourier_encode", ops._dev(xd), c_i64(5), ops._dev(bd), ops._dev(ad), c_i(freq), c_f(1.0),
        c_i(1 if inc else 0), ops._dev(out)), 5 * width, "wider than 4096")
    with pytest.raises(FfnError, match="2048 frequencies, 2046 with include_input"):
        ops.fourier_encode(xd, bd, ad, 1.0, inc)


def test_entry_point_refusals_launch_nothing():
    freq, n = 6, 9
    x, b, a = _inputs(freq, n, 1)
    xd, bd, ad = x.to(dev()), b.contiguous().to(dev()), a.to(dev())
    null = ops._DevPtr(0)
    floats = n * (2 * freq + 3)

    def entry(x_=None, n_=n, b_=None, freq_=freq, out_=None):
        return lambda out, buf: ops._call(
            "ffn_fourier_encode", ops._dev(xd) if x_ is None else x_, c_i64(n_), ops._dev(bd) if b_ is None else b_,
            ops._dev(ad), c_i(freq_), c_f(1.0), c_i(1), ops._dev(out) if out_ is None else out_(out, buf))

    _nothing_written(entry(x_=null), floats, "null x or out")
    _nothing_written(lambda out, buf: ops._call(
        "ffn_fourier_encode", ops._dev(xd), c_i64(n), ops._dev(bd), ops._dev(ad), c_i(freq), c_f(1.0), c_i(1), null),
        floats, "null x or out")
    _nothing_written(entry(b_=null), floats, "null b")
    _nothing_written(entry(n_=-1), floats, "n < 0")
    _nothing_written(entry(freq_=-1), floats, "num_freq < 0")
    # rows one float past a 16-byte boundary
    _nothing_written(entry(out_=lambda out, buf: _ptr_at(buf, FRONT + 1)), floats + 1, "16-byte aligned")
    # ... which the copy of F = 0 does not need
    got, buf = _encode_raw(xd, None, None, 0, 1.0, False, front=FRONT + 1)
    assert torch.equal(got.view(torch.int32), xd.view(torch.int32)) and _guards_intact(buf, FRONT + 1, 3 * n)


def test_wrapper_refusals_launch_nothing():
    freq, n = 6, 9
    x, b, a = _inputs(freq, n, 2)
    xd, bd, ad = x.to(dev()), b.contiguous().to(dev()), a.to(dev())
    good = ops.fourier_encode(xd, bd, ad, 1.0, True)
    assert good.shape == (n, 15)
    cases = [
        ("x must be \\(N, 3\\)", ValueError, lambda: ops.fourier_encode(xd[:, :2].contiguous(), bd, ad, 1.0, True)),
        ("x must be \\(N, 3\\)", ValueError, lambda: ops.fourier_encode(xd.reshape(-1), bd, ad, 1.0, True)),
        ("b must be \\(3, F\\)", ValueError, lambda: ops.fourier_encode(xd, bd.t().contiguous(), ad, 1.0, True)),
        ("a has 5 values for 6 frequencies", ValueError, lambda: ops.fourier_encode(xd, bd, ad[:5].contiguous(), 1.0, True)),
        ("a has 7 values for 6 frequencies", ValueError,
         lambda: ops.fourier_encode(xd, bd, torch.ones(7, device=dev()), 1.0, True)),
        ("different devices", RuntimeError, lambda: ops.fourier_encode(xd, b.contiguous(), ad, 1.0, True)),
        ("different devices", RuntimeError, lambda: ops.fourier_encode(xd, bd, a, 1.0, True)),
    ]
    before = good.clone()
    for match, error, call in cases:
        with pytest.raises(error, match=match):
            call()
    torch.cuda.synchronize()
    assert torch.equal(good, before)


# ------------------------------------------------------------------------------------------ K8
def _to_image(colors, ids, width, height):
    """The entry point itself on numpy colours (n, 3) and pixel ids, into a 0x77-filled frame
    between guard bytes: (H, W, 3) uint8 numpy."""
    cd = torch.from_numpy(np.ascontiguousarray(colors, np.float32)).to(dev())
    idd = torch.from_numpy(np.ascontiguousarray(ids, np.int64)).to(dev())
    size = width * height * 3
    buf = torch.full((64 + size + 64,), 0xEE, dtype=torch.uint8, device=dev())
    buf[64:64 + size] = 0x77
    ops._call("ffn_to_image", ops._dev(cd), ops._dev(idd, torch.int64), c_i64(len(ids)), c_i(width), c_i(height),
              _ptr_at(buf, 64))
    torch.cuda.synchronize()
    assert bool((buf[:64] == 0xEE).all()) and bool((buf[64 + size:] == 0xEE).all())
    return buf[64:64 + size].view(height, width, 3).cpu().numpy()


def test_to_image_at_every_quantisation_edge():
    """The 256 levels k / 255 and their float32 neighbours in all three channels of a 16 x 48 frame,
    pixel ids shuffled, over a 0x77 image: the bytes of ``float32(c) * 255`` truncated.  Colours
    outside [0, 256/255) -- NaN, negative, 256/255 and above -- convert to u8 through an int in a
    way C leaves undefined and stay unasserted."""
    ladder = er.quantisation_ladder()
    colors = np.repeat(ladder[:, None], 3, 1)
    ids = np.random.default_rng(0).permutation(768)
    got = _to_image(colors, ids, 48, 16)
    assert np.array_equal(got, er.to_image_bytes(colors, ids, 48, 16))
    assert np.array_equal(_to_image(colors, ids, 48, 16), got)


def test_to_image_row_counts():
    rng = np.random.default_rng(1)
    width, height = 48, 16
    assert not _to_image(np.zeros((0, 3), np.float32), np.zeros((0,), np.int64), width, height).any()
    for n in (1, width * height):
        colors = rng.random((n, 3), dtype=np.float32)
        ids = rng.permutation(width * height)[:n]
        got = _to_image(colors, ids, width, height)
        assert np.array_equal(got, er.to_image_bytes(colors, ids, width, height)), n
        unlisted = np.setdiff1d(np.arange(width * height), ids)
        assert not got.reshape(-1, 3)[unlisted].any()


def test_to_image_past_the_grid_cap():
    """200 001 of the 262 144 pixels of a 512 x 512 frame: 600 003 elements, more than the
    2048 x 256 threads of the capped grid; unlisted pixels are exactly 0."""
    rng = np.random.default_rng(2)
    side, n = 512, 200001
    assert 3 * n > 2048 * 256
    colors = rng.random((n, 3), dtype=np.float32)
    ids = rng.permutation(side * side)[:n]
    got = _to_image(colors, ids, side, side)
    want = er.to_image_bytes(colors, ids, side, side)
    assert np.array_equal(got, want)
    listed = np.zeros(side * side, bool)
    listed[ids] = True
    assert not got.reshape(-1, 3)[~listed].any() and got.reshape(-1, 3)[listed].any()
    assert np.array_equal(_to_image(colors, ids, side, side), got)
    cd, idd = torch.from_numpy(colors).to(dev()), torch.from_numpy(ids).to(dev())
    assert np.array_equal(ops.to_image(cd, idd, side, side).cpu().numpy(), want)


def test_to_image_refusals_leave_the_image_alone():
    width, height, n = 8, 4, 5
    colors = torch.rand(n, 3, device=dev())
    ids = torch.arange(n, dtype=torch.int64, device=dev())
    cp, ip = ops._dev(colors), ops._dev(ids, torch.int64)

    def refused(match, c, i, n_, w, h, image=None):
        size = 3 * width * height
        buf = torch.full((64 + size + 64,), 0xEE, dtype=torch.uint8, device=dev())
        buf[64:64 + size] = 0x77
        frame = buf[64:64 + size]
        with pytest.raises(FfnError, match=match):
            ops._call("ffn_to_image", c, i, c_i64(n_), c_i(w), c_i(h),
                      ops._dev(frame, torch.uint8) if image is None else image)
        torch.cuda.synchronize()
        assert bool((frame == 0x77).all()), match + ": the refused call touched the image"
        assert bool((buf[:64] == 0xEE).all()) and bool((buf[64 + size:] == 0xEE).all())

    refused("width and height must be positive", cp, ip, n, 0, height)
    refused("width and height must be positive", cp, ip, n, width, -1)
    refused("n < 0", cp, ip, -1, width, height)
    refused("n > width \\* height", cp, ip, width * height + 1, width, height)
    refused("null image", cp, ip, n, width, height, image=ops._DevPtr(0))
    refused("null colors or pixel_index", ops._DevPtr(0), ip, n, width, height)
    refused("null colors or pixel_index", cp, ops._DevPtr(0), n, width, height)
    for match, call in (
            ("colors must be \\(n, 3\\)", lambda: ops.to_image(torch.rand(n, 4, device=dev()), ids, width, height)),
            ("colors must be \\(n, 3\\)", lambda: ops.to_image(torch.rand(3 * n, device=dev()), ids, width, height)),
            ("4 pixel ids for 5 colours", lambda: ops.to_image(colors, ids[:4].contiguous(), width, height)),
            ("33 colours for a frame of 8 x 4", lambda: ops.to_image(
                torch.rand(33, 3, device=dev()), torch.arange(33, dtype=torch.int64, device=dev()), width, height)),
            ("must be positive", lambda: ops.to_image(colors, ids, 0, height))):
        with pytest.raises(ValueError, match=match):
            call()


# ------------------------------------------------------------------------------------------ fused render pixels
@pytest.mark.exact_only(reason=FUSED_KERNELS_ARE_EXACT_F32)
@pytest.mark.parametrize("which", ["small", "gaussian512"])
def test_fused_render_writes_the_bytes_of_its_own_colours(golden, which):
    """The u8 frame the fused render kernel writes (one launch over camera 1's ray range, so
    ``pixel_offset != 0``) is K8 of the colours the same launch returns, byte for byte; pixels of
    invalid rays are 0; ``render_image_device`` returns the same bytes.  ``gaussian512`` runs the
    pair-of-waves variant."""
    import fourier_feature_nets_amd as ffn
    from tests.test_kernels_gpu import _load_fourier
    from tests.test_pipeline_gpu import _small_model
    from tests.test_round2_gpu import _scene_sampler
    if which == "small":
        model = _small_model(golden("training"))
    else:
        model, _ = _load_fourier(golden("models"), "gaussian512")
    caster = ffn.Raycaster(model)
    caster.fused_render = "always"
    sampler = _scene_sampler(64)
    assert caster._can_fuse(sampler)
    assert bool(model.program().wide) == (which == "gaussian512")
    width, height, per = sampler.image_width, sampler.image_height, sampler.rays_per_camera
    first = per
    img = torch.zeros((height, width, 3), dtype=torch.uint8, device=dev())
    model.eval()
    with torch.no_grad():
        out = caster.render_rays(sampler, (first, per), image=img, pixel_offset=first, want_color=True)
    local = torch.arange(per, dtype=torch.int64, device=dev())
    keep = sampler.valid[first:first + per] != 0
    assert int(keep.sum()) > 0
    colour = out.color[keep].contiguous()
    assert bool(torch.isfinite(colour).all()) and float(colour.min()) >= 0.0 and float(colour.max()) < 256.0 / 255.0
    want = ops.to_image(colour, local[keep].contiguous(), width, height)
    assert torch.equal(img, want)
    assert np.array_equal(want.cpu().numpy(), er.to_image_bytes(colour.cpu().numpy(), local[keep].cpu().numpy(), width, height))
    assert not bool(img.view(-1, 3)[~keep].any())
    assert int(img.max()) > 0
    assert torch.equal(caster.render_image_device(sampler, 1, 100), img)
