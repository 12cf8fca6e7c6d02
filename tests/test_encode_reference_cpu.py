"""The references of tests/encode_reference.py against the oracle, with teeth, and the proof that
the GPU tests' shape list reaches every branch of K3's launch plan.  No GPU needed."""

import math

import numpy as np
import pytest
import torch

from oracle import ffn_oracle as orc
from tests import encode_reference as er


def _t(a):
    return torch.from_numpy(np.asarray(a))


def _golden_cases(g):
    """(name, x, b, a, scale, include_input, the oracle's float32 features)."""
    x = _t(g["x"])
    out = []
    for name in ("positional", "gaussian"):
        b, a = _t(g[name + "/b_values"]), _t(g[name + "/a_values"])
        out.append((name, x, b, a, math.pi, False, orc.fourier_features(x, a, b)))
        # (the golden amplitudes are all 1: the same inputs again with amplitudes in [0.5, 2])
        gen = torch.Generator().manual_seed(len(name))
        a = torch.rand(b.shape[1], generator=gen) * 1.5 + 0.5
        out.append((name + "+a", x, b, a, math.pi, False, orc.fourier_features(x, a, b)))
    b = _t(g["nerf/pos_encoding"])
    out.append(("nerf", x, b, None, 1.0, True, orc.nerf_encode(x, b, True)))
    return out


def test_reference_agrees_with_the_oracle(golden):
    for name, x, b, a, scale, inc, oracle in _golden_cases(golden("models")):
        ref, terms = er.encode_features(x, b, a, scale, inc)
        assert ref.dtype == torch.float64 and ref.shape == oracle.shape == terms.shape
        worst, failures = er.check_features(name, oracle, ref, terms)
        print("oracle against the float64 reference: %s worst ratio %.3g" % (name, worst))
        assert not failures, "\n".join(failures)


def test_no_frequencies_is_the_input():
    x = torch.rand(7, 3) * 2 - 1
    for b in (None, torch.zeros((3, 0))):
        for inc in (False, True):
            ref, terms = er.encode_features(x, b, None, 2.0, inc)
            assert torch.equal(ref, x.double()) and torch.equal(terms, x.double().abs())
    ones = torch.ones(5)
    b = torch.randn(3, 5)
    assert torch.equal(er.encode_features(x, b, None, 1.5, True)[0], er.encode_features(x, b, ones, 1.5, True)[0])


def test_budget_has_teeth(golden):
    """A scale off by 1e-3, swapped cos / sin blocks and a dropped amplitude each fail the budget
    that the oracle's own float32 features pass."""
    seen_amplitude = False
    for name, x, b, a, scale, inc, oracle in _golden_cases(golden("models")):
        freq = b.shape[1]
        ref, terms = er.encode_features(x, b, a, scale, inc)
        assert not er.check_features(name, oracle, ref, terms)[1]
        off, _ = er.encode_features(x, b, a, scale * (1 + 1e-3), inc)
        assert er.check_features(name, oracle, off, terms)[1], name + ": a scale off by 1e-3 passed"
        swapped = torch.cat([ref[:, freq:2 * freq], ref[:, :freq], ref[:, 2 * freq:]], 1)
        assert er.check_features(name, oracle, swapped, terms)[1], name + ": swapped cos / sin blocks passed"
        if a is not None and bool((a != 1).any()):
            seen_amplitude = True
            bare, bare_terms = er.encode_features(x, b, None, scale, inc)
            assert er.check_features(name, oracle, bare, terms)[1], name + ": a dropped amplitude passed"
            assert er.check_features(name, oracle, bare, bare_terms)[1]
    assert seen_amplitude, "no golden encoding has an amplitude other than 1"


def test_shape_list_reaches_every_branch_of_the_plan():
    cases = er.shape_cases()
    plans = [(f, inc, n, er.encode_plan(f, inc)) for f, inc, n in cases]
    assert all(p is not None for _, _, _, p in plans)
    kernel = [(f, inc, n, p) for f, inc, n, p in plans if not p["copy"]]

    def some(what, cond):
        assert any(cond(f, inc, n, p) for f, inc, n, p in kernel), "no case with " + what

    assert any(p["copy"] for _, _, _, p in plans), "no device-to-device copy case"
    some("lanes == 1", lambda f, inc, n, p: p["lanes"] == 1)
    some("idle threads beside several samples", lambda f, inc, n, p: p["idle"] > 0 and p["spb"] > 1)
    some("idle threads beside one sample", lambda f, inc, n, p: p["idle"] > 0 and p["spb"] == 1)
    some("no idle threads", lambda f, inc, n, p: p["idle"] == 0)
    some("pairs > 256 (a thread loops over slots)", lambda f, inc, n, p: p["pairs"] > 256 and p["slots"] > 1)
    some("an odd frequency count", lambda f, inc, n, p: p["repeats_frequency"])
    some("slots that repeat pair 0", lambda f, inc, n, p: p["repeats_pair"])
    some("group 128", lambda f, inc, n, p: p["group"] == 128 and p["rule"] == "cap")
    some("4 < group < 128", lambda f, inc, n, p: 4 < p["group"] < 128)
    some("group 4 from the 32 KB rule", lambda f, inc, n, p: p["group"] == 4 and p["rule"] == "32KB")
    some("group 4 from the 64 KB rule", lambda f, inc, n, p: p["group"] == 4 and p["rule"] == "64KB")
    some("a tile plus static LDS above 64 KiB", lambda f, inc, n, p: p["lds"] > 65536)
    some("the largest tile", lambda f, inc, n, p: p["lds_dynamic"] == er.TILE_BYTES)
    # the scalar store tail: a last group whose float count is no multiple of four
    some("a scalar store tail", lambda f, inc, n, p: n > 0 and ((n % p["group"]) * p["width"]) % 4 != 0)
    for tail in (1, 2, 3):
        some("%d floats in the scalar tail" % tail,
             lambda f, inc, n, p: n > 0 and ((n % p["group"]) * p["width"]) % 4 == tail)
    some("several groups per block", lambda f, inc, n, p: er.grid_strides(f, inc, n))
    some("n = 0", lambda f, inc, n, p: n == 0)
    some("n below, at and above one group", lambda f, inc, n, p: n == p["group"] - 1)
    some("n at one group", lambda f, inc, n, p: n == p["group"])
    some("n above one group", lambda f, inc, n, p: n == p["group"] + 1)
    # refused: too wide by one frequency for either value of include_input, and the widest that fit
    for f, inc in er.TOO_WIDE:
        assert er.encode_plan(f, inc) is None and er.encode_plan(f - 1, inc) is not None
    assert er.encode_plan(2048, False, lds_limit=65536) is None           # 65536 + 1536 B
    assert er.encode_plan(2048, False, lds_limit=65536 + 1536) is not None
    # without pass-through columns the need passes 64 KiB from F = 2001 upward
    assert er.encode_plan(2000, False, lds_limit=65536)["lds"] == 65536 and er.encode_plan(2001, False, lds_limit=65536) is None


def test_plan_arithmetic_on_known_shapes():
    """The two shapes the kernel's own comments quote: 510 columns (tiny model) and 63 (NeRF)."""
    tiny = er.encode_plan(255, False)
    assert (tiny["width"], tiny["group"], tiny["lanes"], tiny["spb"], tiny["idle"]) == (510, 16, 128, 2, 0)
    nerf = er.encode_plan(30, True)
    assert (nerf["width"], nerf["group"], nerf["lanes"], nerf["spb"], nerf["idle"]) == (63, 128, 15, 17, 1)


def test_truncation_is_load_bearing_and_the_float32_product_is_not():
    """The 768-value ladder against ``floor(float64(c) * 255)``: the bytes differ in exactly one
    value, the float32 just below 0 (truncated to 0, floored to -1 = byte 255), which lies
    outside K8's domain; clipped to [0, 1 + 2^-23] the two agree in every byte, because the
    float32 product of a float32 colour never rounds up onto a level (module docstring of
    tests/encode_reference.py).  The reference therefore truncates a float32 product, as the
    kernels do, and on the clipped ladder its bytes are the exact floor: they can be required
    exactly."""
    ids = np.arange(768)

    def both(ladder):
        colors = np.repeat(ladder[:, None], 3, 1)
        return er.to_image_bytes(colors, ids, 48, 16), er.to_image_bytes_float64(colors, ids, 48, 16), colors

    raw = er.quantisation_ladder(clip=False)
    assert raw.shape == (768,) and raw.dtype == np.float32 and raw[0] < 0 and raw[1] == 0
    exact, floor64, _ = both(raw)
    differ = (exact != floor64).any(axis=2).reshape(-1)
    print("unclipped ladder values whose byte differs from the float64 floor: %d of 768" % int(differ.sum()))
    assert differ.sum() >= 1
    assert differ.nonzero()[0].tolist() == [0]
    assert exact.reshape(-1, 3)[0].tolist() == [0, 0, 0] and floor64.reshape(-1, 3)[0].tolist() == [255, 255, 255]

    ladder = er.quantisation_ladder()
    assert ladder.shape == (768,) and ladder.dtype == np.float32
    assert ladder.min() == 0.0 and ladder.max() == np.float32(1) + np.float32(2.0 ** -23)
    exact, floor64, colors = both(ladder)
    assert exact.shape == (16, 48, 3) and exact.dtype == np.uint8
    assert np.array_equal(exact, floor64)
    # the neighbour below a level is one level down, the level and its neighbour above are on it
    k = np.arange(256)
    want = np.stack([np.maximum(k - 1, 0), k, k], 1).reshape(-1)
    assert np.array_equal(exact.reshape(-1, 3), np.repeat(want[:, None], 3, 1).astype(np.uint8))
    # the oracle's own (x * 255).astype(uint8) agrees
    assert np.array_equal(exact, orc.to_image(ids, colors, 48, 16))


def test_float32_product_never_rounds_up_onto_a_level():
    """For every level m the largest float32 below m / 255 still truncates to m - 1 (its exact
    product is at least half an ulp of m below m), and the float32 nearest m / 255 is not below
    it: no float32 colour in [0, 1] gets another byte from the float32 product than from the
    exact one."""
    m = np.arange(1, 256)
    level = (m / 255.0).astype(np.float32)
    assert bool((level.astype(np.float64) * 255.0 >= m).all())          # (24 x 8 bits: exact in float64)
    below = np.nextafter(level, np.float32(-1), dtype=np.float32)
    assert bool((below.astype(np.float64) * 255.0 < m).all())
    assert np.array_equal((below * np.float32(255)).astype(np.int32), m - 1)
    assert np.array_equal((level * np.float32(255)).astype(np.int32), m)


def test_to_image_bytes_scatters_and_leaves_the_rest_zero():
    colors = np.array([[0.5, 0.25, 1.0], [0.0, 0.999, 0.1]], np.float32)
    img = er.to_image_bytes(colors, np.array([5, 2]), 4, 2)
    flat = img.reshape(-1, 3)
    assert flat[5].tolist() == [127, 63, 255] and flat[2].tolist() == [0, 254, 25]
    assert int(np.delete(flat, [2, 5], 0).sum()) == 0
    assert er.to_image_bytes(np.zeros((0, 3), np.float32), np.zeros((0,), np.int64), 4, 2).sum() == 0
